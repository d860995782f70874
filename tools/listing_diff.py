"""Are the kernels of two device listings the same code?  For a change that must not touch device code (a host refactor):
    hipcc <the flags of _lib.build> --cuda-device-only -S brief_pytorch_amd/csrc/brief_hip.hip -o a.s      (once per commit)
    python tools/listing_diff.py a.s b.s
Per kernel: the instruction list (comments stripped, .LBBn_ labels normalised) and the .amdhsa_* resource lines must be equal.  Prints
the kernels that differ with their instruction counts, VGPRs, SGPRs, scratch and LDS, and whether the kernels come in the same order."""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    code, order = {}, []
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines = []
        for ln in m.group(2).split("\n"):
            ln = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r";.*", "", ln).rstrip())
            if ln.strip():
                lines.append(ln)
        code[m.group(1)] = lines
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        res[m.group(1)] = [ln.strip() for ln in m.group(2).split("\n") if ln.strip().startswith(".amdhsa_")]
        order.append(m.group(1))
    return code, res, order


def field(res, key):
    return next((ln.split()[1] for ln in res if ln.startswith(".amdhsa_" + key + " ")), "?")


a_code, a_res, a_order = kernels(sys.argv[1])
b_code, b_res, b_order = kernels(sys.argv[2])
same = 0
for k in a_order:
    if k not in b_res:
        print("MISSING in %s: %s" % (sys.argv[2], k))
    elif a_code[k] == b_code[k] and a_res[k] == b_res[k]:
        same += 1
    else:
        name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
        what = [(len(c[k]),) + tuple(field(r[k], f) for f in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size"))
                for c, r in ((a_code, a_res), (b_code, b_res))]
        print("DIFFERS %s: (instructions, vgpr, sgpr, scratch, lds) %s -> %s" % (name[:90], what[0], what[1]))
for k in b_order:
    if k not in a_res:
        print("NEW in %s: %s" % (sys.argv[2], k))
print("kernels %d / %d, identical %d, same order: %s" % (len(a_order), len(b_order), same, a_order == b_order))
