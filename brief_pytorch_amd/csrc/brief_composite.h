// brief_composite.h — the arithmetic of the composite view (brief_pytorch_amd/composite.py, csrc/brief_composite.inc), defined once:
// the scalar functions the gfx950 kernels call, compiled on the host too (brief_view_composite_host, tests/test_composite_host.py).
//
// Front-to-back emission-absorption compositing, C += T * alpha * c; T *= 1 - alpha, is order-dependent, and in floats not even
// associative.  Here it is taken to the LOG DOMAIN and to integers, so that it is a pair of sums:
//     classification  a sample's value v (one channel of the integer decode) indexes the transfer table tf, int32 [2^b][4] =
//                     (tau, eR, eG, eB), at v >> (bits of the dtype - b).  tau is the sample's optical depth in units of 2^-16
//                     octaves: the sample multiplies the transmittance by 2^(-tau / 65536); 0 <= tau <= TAU_SAT = 32 * 65536, and
//                     TAU_SAT is opaque.  e_c = round(256 * colour_c * (1 - 2^(-tau / 65536))), 0 .. 65280, is the premultiplied
//                     emission (composite.make_transfer computes it from the already quantised tau).
//     prefix          P_i = min(sum of tau over the inside samples before i, TAU_SAT): a sum of non-negative integers, exact in any
//                     order, and the saturation commutes with it: min(min(x, S) + y, S) = min(x + y, S) for x, y >= 0.
//     weight          W(P), the transmittance 2^(-P / 65536) in Q0.32: a pure integer function (brief_composite_w), W(0) = 2^32,
//                     W(TAU_SAT) = 0, non-increasing.
//     accumulate      acc_c = sum over the inside samples of W(P_i) * e_c(i), uint64: exact in any order.
//     finish          out_c = min(255, (acc_c + bg_c * 256 * W(P_total) + 2^39) >> 40), A = min(255, ((2^32 - W(P_total)) * 255 + 2^31) >> 32)
// Nothing depends on how the samples of a ray are dealt to lanes, chunks or launches: only on their order along the ray, which is k.
//
// W.  With q = P >> 16 and f = P & 0xFFFF: W = 0 for q >= 32, else ((A[f >> 8] * B[f & 255]) >> 30) >> q, A[i] = round(2^31 * 2^(-i / 256)),
// B[j] = round(2^31 * 2^(-j / 65536)).  A[0] = B[0] = 2^31, so W(0) = 2^62 >> 30 = 2^32 exactly.  Each table entry is within half a
// unit of its real and at most 2^31, so the product is within 2^31 + 1/4 of the real 2^62 * 2^(-f / 65536): within 2 + 2^-32 after the
// division by 2^30, and each of the two floors takes less than 1, so |W(P) - 2^32 * 2^(-P / 65536)| < 4 =: delta.
//
// acc_c FITS 64 BITS for a ray of up to 2^24 - 1 samples under a table of make_transfer.  There e <= 65280 * alpha + 1/2 with
// alpha = 1 - 2^(-tau / 65536); e = 0 for tau = 0, and for tau >= 1 alpha >= 1 - 2^(-1 / 65536) > 1.0576e-5, so 1/2 < 0.725 * 65280 * alpha
// and e < 2^17 * alpha: the rounding of e is bounded PER TERM by a factor, not by a constant.  Real weights telescope:
// 2^32 * 2^(-P_i / 65536) * alpha_i = Wr(P_i) - Wr(P_i + tau_i), and a saturated prefix has W = 0, so
//     acc_c < 2^17 * sum (Wr(P_i) + delta) * alpha_i <= 2^17 * (2^32 + delta * 2^24) < 2^50,
// and the finish adds at most 65280 * 2^32 + 2^39 < 2^48.  A table that is merely in range (the entries' own limits are all the
// host-visible entries check) may pair a large e with tau = 0; then acc_c wraps modulo 2^64, on the device and on the host alike.
//
// SHADED composite (brief_view_composite_select / _pick / _shade_fold, brief_view_composite_shade_host).  Opacity is not touched: tau,
// P_i, hits, tau_run and A are the plain composite's.  Only a sample's emission is scaled, by a two-sided Lambert term s = KA + KD *
// |n . l|, n = g / |g|, g the physical gradient of the classified channel (the net's analytic Jacobian times gscale) and l the unit
// direction the light travels.  Every fp32 operation rounds on its own, nothing is contracted, sqrt and division are the correctly
// rounded ones on the device as on the host:
//     g_a  = fl(j_a * gscale_a)
//     d    = fl(fl(fl(g0 * l0) + fl(g1 * l1)) + fl(g2 * l2)),   q = fl(fl(fl(g0 * g0) + fl(g1 * g1)) + fl(g2 * g2)),   len = sqrt(q)
//     c_q  = 256 where len is not a finite positive number (a sample without a gradient direction is lit fully), else
//            min(256, (int)fl(fl(fl(|d| / len) * 256) + 0.5)); a term that is not below 256 as a float (a NaN from a light far from
//            unit length among them) is 256
//     s_q  = min(256, ka_q + ((kd_q * c_q + 128) >> 8)),   ka_q = round(256 * KA), kd_q = round(256 * KD), 0 .. 256, from the host
//     e'_c = (e_c * s_q + 128) >> 8,   acc_c += W(P_i) * e'_c
// s_q <= 256, so e'_c <= e_c (e_c * 256 + 128 < 2^32): every term is at most the plain composite's and the 64-bit bound above still
// holds.  ka_q = 256, kd_q = 0 gives s_q = 256 and e' = e: the plain composite, whatever the Jacobian holds.
// A sample NEEDS a gradient iff it is inside the clip box, its table row has eR | eG | eB != 0 and P_i < TAU_SAT
// (brief_composite_need): every other sample contributes 0 whatever its shade (e = 0, or W(P_i) = 0 for a saturated prefix).  The rule
// reads integers only, so the selection depends on a sample's place along its ray alone, as the image does.
#pragma once
#include <stdint.h>
#include "brief_view.h"

#define BRIEF_COMPOSITE_TAU_SAT (32 << 16)
#define BRIEF_COMPOSITE_E_MAX 65280

// the transmittance 2^(-tau / 65536) in Q0.32, 0 <= tau <= TAU_SAT (anything above is opaque too)
BRIEF_HD uint64_t brief_composite_w(uint32_t tau)
{
    static const uint32_t A[256] = {
        2147483648u, 2141676973u, 2135885998u, 2130110682u, 2124350982u, 2118606857u, 2112878262u, 2107165158u,
        2101467502u, 2095785251u, 2090118366u, 2084466803u, 2078830522u, 2073209480u, 2067603638u, 2062012954u,
        2056437387u, 2050876895u, 2045331439u, 2039800978u, 2034285470u, 2028784876u, 2023299156u, 2017828268u,
        2012372174u, 2006930832u, 2001504204u, 1996092249u, 1990694927u, 1985312200u, 1979944027u, 1974590370u,
        1969251188u, 1963926443u, 1958616096u, 1953320108u, 1948038440u, 1942771053u, 1937517909u, 1932278970u,
        1927054196u, 1921843549u, 1916646992u, 1911464486u, 1906295993u, 1901141476u, 1896000896u, 1890874216u,
        1885761398u, 1880662405u, 1875577199u, 1870505744u, 1865448001u, 1860403934u, 1855373507u, 1850356681u,
        1845353420u, 1840363688u, 1835387448u, 1830424663u, 1825475297u, 1820539314u, 1815616678u, 1810707353u,
        1805811301u, 1800928489u, 1796058879u, 1791202437u, 1786359126u, 1781528911u, 1776711757u, 1771907628u,
        1767116489u, 1762338305u, 1757573041u, 1752820662u, 1748081133u, 1743354420u, 1738640488u, 1733939301u,
        1729250827u, 1724575029u, 1719911875u, 1715261330u, 1710623359u, 1705997930u, 1701385007u, 1696784557u,
        1692196547u, 1687620943u, 1683057710u, 1678506817u, 1673968228u, 1669441912u, 1664927835u, 1660425963u,
        1655936265u, 1651458706u, 1646993254u, 1642539877u, 1638098541u, 1633669214u, 1629251865u, 1624846459u,
        1620452965u, 1616071351u, 1611701585u, 1607343634u, 1602997467u, 1598663052u, 1594340357u, 1590029350u,
        1585730000u, 1581442275u, 1577166143u, 1572901575u, 1568648537u, 1564406999u, 1560176931u, 1555958300u,
        1551751076u, 1547555228u, 1543370725u, 1539197537u, 1535035634u, 1530884983u, 1526745556u, 1522617322u,
        1518500250u, 1514394310u, 1510299473u, 1506215708u, 1502142985u, 1498081275u, 1494030547u, 1489990772u,
        1485961921u, 1481943963u, 1477936870u, 1473940611u, 1469955159u, 1465980482u, 1462016553u, 1458063343u,
        1454120821u, 1450188960u, 1446267730u, 1442357104u, 1438457051u, 1434567544u, 1430688553u, 1426820052u,
        1422962010u, 1419114401u, 1415277195u, 1411450365u, 1407633882u, 1403827719u, 1400031848u, 1396246240u,
        1392470869u, 1388705706u, 1384950723u, 1381205894u, 1377471191u, 1373746586u, 1370032052u, 1366327563u,
        1362633090u, 1358948606u, 1355274085u, 1351609500u, 1347954824u, 1344310030u, 1340675091u, 1337049980u,
        1333434672u, 1329829140u, 1326233356u, 1322647296u, 1319070932u, 1315504238u, 1311947188u, 1308399756u,
        1304861917u, 1301333643u, 1297814910u, 1294305692u, 1290805962u, 1287315695u, 1283834865u, 1280363448u,
        1276901417u, 1273448747u, 1270005413u, 1266571390u, 1263146652u, 1259731174u, 1256324931u, 1252927899u,
        1249540052u, 1246161366u, 1242791816u, 1239431376u, 1236080024u, 1232737732u, 1229404479u, 1226080238u,
        1222764986u, 1219458698u, 1216161350u, 1212872918u, 1209593378u, 1206322705u, 1203060876u, 1199807867u,
        1196563654u, 1193328213u, 1190101520u, 1186883552u, 1183674286u, 1180473697u, 1177281762u, 1174098458u,
        1170923762u, 1167757650u, 1164600099u, 1161451085u, 1158310587u, 1155178580u, 1152055042u, 1148939949u,
        1145833280u, 1142735011u, 1139645120u, 1136563583u, 1133490379u, 1130425485u, 1127368878u, 1124320536u,
        1121280436u, 1118248556u, 1115224875u, 1112209370u, 1109202018u, 1106202798u, 1103211687u, 1100228665u,
        1097253708u, 1094286796u, 1091327906u, 1088377016u, 1085434106u, 1082499153u, 1079572136u, 1076653033u};
    static const uint32_t B[256] = {
        2147483648u, 2147460935u, 2147438222u, 2147415510u, 2147392798u, 2147370086u, 2147347374u, 2147324663u,
        2147301951u, 2147279240u, 2147256530u, 2147233819u, 2147211109u, 2147188399u, 2147165689u, 2147142979u,
        2147120270u, 2147097561u, 2147074852u, 2147052143u, 2147029435u, 2147006727u, 2146984019u, 2146961311u,
        2146938604u, 2146915897u, 2146893190u, 2146870483u, 2146847777u, 2146825071u, 2146802365u, 2146779659u,
        2146756953u, 2146734248u, 2146711543u, 2146688838u, 2146666134u, 2146643430u, 2146620726u, 2146598022u,
        2146575318u, 2146552615u, 2146529912u, 2146507209u, 2146484506u, 2146461804u, 2146439102u, 2146416400u,
        2146393698u, 2146370997u, 2146348296u, 2146325595u, 2146302894u, 2146280194u, 2146257494u, 2146234794u,
        2146212094u, 2146189395u, 2146166695u, 2146143996u, 2146121298u, 2146098599u, 2146075901u, 2146053203u,
        2146030505u, 2146007807u, 2145985110u, 2145962413u, 2145939716u, 2145917019u, 2145894323u, 2145871627u,
        2145848931u, 2145826236u, 2145803540u, 2145780845u, 2145758150u, 2145735455u, 2145712761u, 2145690067u,
        2145667373u, 2145644679u, 2145621986u, 2145599292u, 2145576599u, 2145553907u, 2145531214u, 2145508522u,
        2145485830u, 2145463138u, 2145440446u, 2145417755u, 2145395064u, 2145372373u, 2145349683u, 2145326992u,
        2145304302u, 2145281612u, 2145258923u, 2145236233u, 2145213544u, 2145190855u, 2145168166u, 2145145478u,
        2145122790u, 2145100102u, 2145077414u, 2145054727u, 2145032039u, 2145009352u, 2144986666u, 2144963979u,
        2144941293u, 2144918607u, 2144895921u, 2144873235u, 2144850550u, 2144827865u, 2144805180u, 2144782496u,
        2144759811u, 2144737127u, 2144714443u, 2144691760u, 2144669076u, 2144646393u, 2144623710u, 2144601027u,
        2144578345u, 2144555663u, 2144532981u, 2144510299u, 2144487618u, 2144464936u, 2144442255u, 2144419575u,
        2144396894u, 2144374214u, 2144351534u, 2144328854u, 2144306175u, 2144283495u, 2144260816u, 2144238137u,
        2144215459u, 2144192780u, 2144170102u, 2144147424u, 2144124747u, 2144102069u, 2144079392u, 2144056715u,
        2144034038u, 2144011362u, 2143988686u, 2143966010u, 2143943334u, 2143920659u, 2143897983u, 2143875308u,
        2143852634u, 2143829959u, 2143807285u, 2143784611u, 2143761937u, 2143739263u, 2143716590u, 2143693917u,
        2143671244u, 2143648572u, 2143625899u, 2143603227u, 2143580555u, 2143557884u, 2143535212u, 2143512541u,
        2143489870u, 2143467199u, 2143444529u, 2143421859u, 2143399189u, 2143376519u, 2143353850u, 2143331180u,
        2143308511u, 2143285843u, 2143263174u, 2143240506u, 2143217838u, 2143195170u, 2143172502u, 2143149835u,
        2143127168u, 2143104501u, 2143081834u, 2143059168u, 2143036502u, 2143013836u, 2142991170u, 2142968505u,
        2142945840u, 2142923175u, 2142900510u, 2142877846u, 2142855181u, 2142832518u, 2142809854u, 2142787190u,
        2142764527u, 2142741864u, 2142719201u, 2142696539u, 2142673876u, 2142651214u, 2142628553u, 2142605891u,
        2142583230u, 2142560569u, 2142537908u, 2142515247u, 2142492587u, 2142469927u, 2142447267u, 2142424607u,
        2142401948u, 2142379288u, 2142356629u, 2142333971u, 2142311312u, 2142288654u, 2142265996u, 2142243338u,
        2142220681u, 2142198024u, 2142175367u, 2142152710u, 2142130053u, 2142107397u, 2142084741u, 2142062085u,
        2142039429u, 2142016774u, 2141994119u, 2141971464u, 2141948809u, 2141926155u, 2141903501u, 2141880847u,
        2141858193u, 2141835540u, 2141812887u, 2141790234u, 2141767581u, 2141744929u, 2141722276u, 2141699624u};
    const uint32_t q = tau >> 16, f = tau & 0xFFFFu;
    if (q >= 32u) return 0;
    return (((uint64_t)A[f >> 8] * (uint64_t)B[f & 255u]) >> 30) >> q;
}

// min(a + b, TAU_SAT) for a <= TAU_SAT and b < 2^31 - TAU_SAT (a pass of 64 lanes adds at most 64 * TAU_SAT = 2^27)
BRIEF_HD uint32_t brief_composite_add(uint32_t a, uint32_t b)
{
    const uint32_t s = a + b;
    return s < (uint32_t)BRIEF_COMPOSITE_TAU_SAT ? s : (uint32_t)BRIEF_COMPOSITE_TAU_SAT;
}

// the pixel from its folded state: RGB composited over the background bg (0 .. 255 per channel), and the opacity A
BRIEF_HD void brief_composite_pixel(uint32_t tau_total, const uint64_t acc[3], const int32_t bg[3], uint8_t out[4])
{
    const uint64_t w = brief_composite_w(tau_total);
    for (int c = 0; c < 3; ++c) {
        const uint64_t y = (acc[c] + (uint64_t)bg[c] * 256u * w + ((uint64_t)1 << 39)) >> 40;
        out[c] = (uint8_t)(y < 255u ? y : 255u);
    }
    const uint64_t a = ((((uint64_t)1 << 32) - w) * 255u + ((uint64_t)1 << 31)) >> 32;
    out[3] = (uint8_t)(a < 255u ? a : 255u);
}

// ---- the SHADED composite: the Lambert term of a sample in Q8, and the rule that says which samples need one.
// sqrtf and `/` are IEEE-correctly rounded in device code (clang's default for HIP, -fhip-fp32-correctly-rounded-divide-sqrt) as they
// are on the host; __fsqrt_rn is NOT used: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers define it as the native, 1-ulp sqrt.

// c_q = round(256 * |cos(g, light)|) of g_a = j_a * gscale_a, 0 .. 256; 256 where g has no direction
BRIEF_HD int32_t brief_composite_cos_q(const float j[3], const float gscale[3], const float light[3])
{
    BRIEF_VIEW_NO_CONTRACT
    const float g0 = j[0] * gscale[0];
    const float g1 = j[1] * gscale[1];
    const float g2 = j[2] * gscale[2];
    const float d0 = g0 * light[0];
    const float d1 = g1 * light[1];
    const float d2 = g2 * light[2];
    const float d01 = d0 + d1;
    const float d = d01 + d2;
    const float q0 = g0 * g0;
    const float q1 = g1 * g1;
    const float q2 = g2 * g2;
    const float q01 = q0 + q1;
    const float q = q01 + q2;
    const float len = __builtin_sqrtf(q);
    if (!(len > 0.f) || len - len != 0.f) return 256;
    const float c = __builtin_fabsf(d) / len;
    const float t = c * 256.f;
    const float u = t + 0.5f;
    return u < 256.f ? (int32_t)u : 256;                         // (u >= 0 or NaN here)
}

// s_q, the factor of a sample's emission in Q8, 0 .. 256 for ka_q, kd_q in 0 .. 256
BRIEF_HD int32_t brief_composite_shade_q(const float j[3], const float gscale[3], const float light[3], int32_t ka_q, int32_t kd_q)
{
    const int32_t s = ka_q + ((kd_q * brief_composite_cos_q(j, gscale, light) + 128) >> 8);
    return s < 256 ? s : 256;
}

// e' = (e * s_q + 128) >> 8 <= e
BRIEF_HD uint32_t brief_composite_lit(uint32_t e, int32_t s_q) { return (e * (uint32_t)s_q + 128u) >> 8; }

// whether a sample can reach the pixel, so that its shade matters: inside the clip box, emitting, and in front of saturation
BRIEF_HD bool brief_composite_need(bool inside, uint32_t er, uint32_t eg, uint32_t eb, uint32_t prefix)
{
    return inside && (er | eg | eb) != 0u && prefix < (uint32_t)BRIEF_COMPOSITE_TAU_SAT;
}

// ---- the composite of a PARTITION (one net per block, view.render_partition's ownership): carry the prefix across blocks.
// Per pixel and block the owned samples form one interval of k (brief_view_part_ray_range), a SEGMENT; the segments of a pixel are
// disjoint, so their k0 order them front to back.  A block's window rays carry the state of its segments: hits_w, tau_w (the
// segment's saturated total T after the first pass) and acc_w[3] (its colour sums under carry-in 0).  The weight of a sample is
// W(min(C + L, TAU_SAT)), L the optical depth in front of it inside its own segment and C = min(sum of T over the segments in front,
// TAU_SAT); the saturation commutes with the sum, so a segment folds on its own once C is known.  C == 0: the first pass is already
// final.  C == TAU_SAT: the segment contributes nothing.  Otherwise it is folded a second time with carry-in C.
// The window rays of all blocks lie in one block-major array; brief_composite_window (include/brief_hip.h) names a block's slice of it.
// The functions below trust the table: bases 0 and then each the end of the slice before, windows inside the image.  The host entries
// check it entry by entry before they call them; a device table cannot be read before a launch, and a malformed one is undefined behaviour.

// the window ray of pixel (row, col) in the block's slice, or -1 where the window does not hold the pixel
BRIEF_HD int64_t brief_composite_window_ray(const brief_composite_window &b, int32_t row, int32_t col)
{
    const int32_t wr = row - b.row0, wc = col - b.col0;
    if (wr < 0 || wc < 0 || wr >= b.wrows || wc >= b.wcols) return -1;
    return b.base + (int64_t)wr * b.wcols + wc;
}

// the block whose slice holds window ray w, 0 <= w < window_rays: the last one whose base is <= w (an empty window holds no ray)
BRIEF_HD int32_t brief_composite_window_of(const brief_composite_window *wins, int32_t blocks, int64_t w)
{
    int32_t lo = 0, hi = blocks - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (wins[mid].base <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// C and the second pass's count of window ray w: C = min(sum of tau_w over the segments of the same pixel with a smaller k0, TAU_SAT)
BRIEF_HD void brief_composite_carry(const brief_composite_window *wins, int32_t blocks, const int32_t *k0, const int32_t *cnt,
                                    const int32_t *tau_w, int64_t w, int32_t &carry, int32_t &cnt2)
{
    carry = 0;
    cnt2 = 0;
    const int32_t n = cnt[w];
    if (n <= 0) return;
    const brief_composite_window &own = wins[brief_composite_window_of(wins, blocks, w)];
    const int64_t i = w - own.base;
    const int32_t wr = (int32_t)(i / own.wcols);
    const int32_t row = own.row0 + wr, col = own.col0 + (int32_t)(i - (int64_t)wr * own.wcols), kb = k0[w];
    uint64_t sum = 0;                                            // at most blocks * TAU_SAT < 2^52
    for (int32_t b = 0; b < blocks; ++b) {
        const int64_t x = brief_composite_window_ray(wins[b], row, col);
        if (x < 0 || x == w) continue;
        if (cnt[x] > 0 && k0[x] < kb) sum += (uint64_t)(uint32_t)tau_w[x];
    }
    carry = (int32_t)(sum < (uint64_t)BRIEF_COMPOSITE_TAU_SAT ? sum : (uint64_t)BRIEF_COMPOSITE_TAU_SAT);
    cnt2 = carry > 0 && carry < BRIEF_COMPOSITE_TAU_SAT ? n : 0;
}

// the state of pixel (row, col) from its segments: the first pass's sums where C == 0, the second pass's where 0 < C < TAU_SAT
BRIEF_HD void brief_composite_gather(const brief_composite_window *wins, int32_t blocks, int32_t row, int32_t col,
                                     const int32_t *hits_w, const int32_t *tau_w, const uint64_t *acc_w, const int32_t *carry, const uint64_t *acc_w2,
                                     int32_t &hits, uint32_t &tau_run, uint64_t acc[3])
{
    uint64_t t = 0;
    hits = 0;
    acc[0] = acc[1] = acc[2] = 0;
    for (int32_t b = 0; b < blocks; ++b) {
        const int64_t x = brief_composite_window_ray(wins[b], row, col);
        if (x < 0) continue;
        hits += hits_w[x];
        t += (uint64_t)(uint32_t)tau_w[x];
        const int32_t c = carry[x];
        const uint64_t *a = c == 0 ? acc_w + x * 3 : (c < BRIEF_COMPOSITE_TAU_SAT ? acc_w2 + x * 3 : (const uint64_t *)0);
        if (a)
            for (int j = 0; j < 3; ++j) acc[j] += a[j];
    }
    tau_run = (uint32_t)(t < (uint64_t)BRIEF_COMPOSITE_TAU_SAT ? t : (uint64_t)BRIEF_COMPOSITE_TAU_SAT);
}
