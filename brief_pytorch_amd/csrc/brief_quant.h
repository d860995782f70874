// brief_quant.h — the weight quantiser of the quantised artefact (brief_pytorch_amd/quantize.py), defined once: the scalar functions the
// gfx950 kernels of brief_quant.inc call, compiled on the host too (tests/test_quantize_host.py).
//
// Uniform, affine, per tensor (every weight matrix and every bias is a tensor).  Every fp32 operation rounds on its own:
//     lo = min(w); hi = max(w); top = 2^bits - 1
//     step = fl(fl(hi - lo) / fl(top))
//     code = clamp(rint(fl(fl(w - lo) / step)), 0, top)        (step == 0: code = 0)
//     deq  = fl(fl(code * step) + lo)
// rint rounds ties to even, the division is correctly rounded, and the multiply and the add of deq are never contracted into an fma
// (the pragma below: without it the device code is one v_fma_f32).  Plain numpy float32 arithmetic is then an exact restatement, so
// load_model dequantises on the host and the tests compare bit for bit.
#pragma once

#if defined(__HIPCC__)
#ifndef BRIEF_HD
#define BRIEF_HD __host__ __device__ __forceinline__
#endif
#else
#include <cmath>
#ifndef BRIEF_HD
#define BRIEF_HD static inline
#endif
#endif

#if defined(__clang__)
#define BRIEF_QUANT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define BRIEF_QUANT_NO_CONTRACT      /* g++: built with -ffp-contract=off */
#endif

BRIEF_HD float brief_quant_step(float lo, float hi, int bits)
{
    BRIEF_QUANT_NO_CONTRACT
    const float top = (float)((1 << bits) - 1);
    const float spread = hi - lo;
    return spread / top;
}

// the integer code of w as a float in [0, top]
BRIEF_HD float brief_quant_code(float w, float lo, float step, float top)
{
    BRIEF_QUANT_NO_CONTRACT
    if (step == 0.f) return 0.f;
    const float d = w - lo;
    const float q = rintf(d / step);
    return q < 0.f ? 0.f : (q > top ? top : q);      // (a NaN fails both comparisons and stays: such a tensor is refused before it is written)
}

BRIEF_HD float brief_quant_deq(float code, float lo, float step)
{
    BRIEF_QUANT_NO_CONTRACT
    const float p = code * step;
    return p + lo;
}
