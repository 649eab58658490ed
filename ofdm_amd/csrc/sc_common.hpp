// sc_common.hpp -- what the four Schmidl-Cox files (kernels_sync / _sc80 / _scstream / _scbig.hip) share: the four sliding sums of a
// lag, a candidate for the peak, and the ONE definition of "first maximum wins" that tests/test_gpu_sc_margins.py holds every
// detector to.
#pragma once
#include "device_common.hpp"
#include "wave_ops.hpp"

namespace ofdm {

// P = sum conj(r[m]) r[m + L] (pr, pi), E = sum |r[m]|^2, R = sum |r[m + L]|^2 over one window
struct ScSums { double pr, pi, e, r; };
__device__ __forceinline__ ScSums s_add(ScSums a, ScSums b) { return ScSums{a.pr + b.pr, a.pi + b.pi, a.e + b.e, a.r + b.r}; }
__device__ __forceinline__ ScSums s_shfl_up(ScSums a, int d) {
    return ScSums{__shfl_up(a.pr, d, 64), __shfl_up(a.pi, d, 64), __shfl_up(a.e, d, 64), __shfl_up(a.r, d, 64)};
}
__device__ __forceinline__ ScSums s_shfl_xor(ScSums a, int d) {
    return ScSums{__shfl_xor(a.pr, d, 64), __shfl_xor(a.pi, d, 64), __shfl_xor(a.e, d, 64), __shfl_xor(a.r, d, 64)};
}
// one more product pair of a window, a = r[m], b = r[m + L]: the oracle's four products in the oracle's order (products of f32
// samples are exact in f64, so every step rounds as the oracle's does, fused or not).  By value (`y = acc(y, a, b)`): through a
// reference sc_direct's loop came out with its registers in another order.
__device__ __forceinline__ ScSums acc(ScSums y, cf a, cf b) {
    const double ar = a.x, ai = a.y, br = b.x, bi = b.y;
    y.pr += ar * br + ai * bi;
    y.pi += ar * bi - ai * br;
    y.e += ar * ar + ai * ai;
    y.r += br * br + bi * bi;
    return y;
}
// the oracle's num = |P|^2 (no fused multiply-add: the oracle is compiled without contraction)
__device__ __forceinline__ double sc_num(ScSums y) { return __dadd_rn(__dmul_rn(y.pr, y.pr), __dmul_rn(y.pi, y.pi)); }

// a lag's metric as the fraction num / den, with the P it came from (CFO = arg P / L)
struct ScCand { double num, den, pr, pi; int lag; };
// first maximum wins, whatever the order of discovery: strictly greater replaces; equal replaces only from a lower lag
__device__ __forceinline__ ScCand cand_pick(ScCand a, ScCand b) {
    const double lhs = b.num * a.den, rhs = a.num * b.den;
    return (lhs > rhs || (lhs == rhs && b.lag < a.lag)) ? b : a;
}
// PRECONDITION: every lag a stands for is lower than every lag b stands for.  Then b wins only if strictly greater, and that is
// cand_pick without the lag comparison
__device__ __forceinline__ ScCand cand_pick_ordered(ScCand a, ScCand b) { return (b.num * a.den > a.num * b.den) ? b : a; }
__device__ __forceinline__ ScCand cand_shfl_xor(ScCand a, int d) {
    return ScCand{__shfl_xor(a.num, d, 64), __shfl_xor(a.den, d, 64), __shfl_xor(a.pr, d, 64), __shfl_xor(a.pi, d, 64),
                  __shfl_xor(a.lag, d, 64)};
}
__device__ __forceinline__ ScCand cand_shfl_down(ScCand a, int d) {
    return ScCand{__shfl_down(a.num, d, 64), __shfl_down(a.den, d, 64), __shfl_down(a.pr, d, 64), __shfl_down(a.pi, d, 64),
                  __shfl_down(a.lag, d, 64)};
}
__device__ __forceinline__ ScCand cand_readlane(ScCand c, int l) {
    return ScCand{readlane_d(c.num, l), readlane_d(c.den, l), readlane_d(c.pr, l), readlane_d(c.pi, l), __builtin_amdgcn_readlane(c.lag, l)};
}
template <int CTRL> __device__ __forceinline__ ScCand cand_dpp(ScCand c) {
    return ScCand{dpp_d<CTRL>(c.num), dpp_d<CTRL>(c.den), dpp_d<CTRL>(c.pr), dpp_d<CTRL>(c.pi), dpp_i<CTRL>(c.lag)};
}
// first maximum over the wavefront, in every lane
__device__ __forceinline__ ScCand cand_wave_best(ScCand c) {
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) c = cand_pick(c, cand_shfl_xor(c, sft));
    return c;
}

} // namespace ofdm
