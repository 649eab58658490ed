// wave_ops.hpp -- the wave64 vocabulary of the gfx950 kernels: waits and fences, DPP moves, wavefront scans and reductions, lane reads.
// One definition each; nothing here knows about OFDM or Schmidl-Cox (what the four Schmidl-Cox files share is sc_common.hpp).
#pragma once
#include <hip/hip_runtime.h>

namespace ofdm {

// ---- waits and fences
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// wavefront-scope fence: this wavefront's LDS accesses in front of it stay in front of those behind it (lanes exchange data through LDS without a barrier)
__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// A value the compiler must KEEP in a VGPR and cannot see through: a per-lane constant is not rematerialised inside the loop, and
// an index that adds pinned(0) keeps a wave-uniform load a per-lane load (as a scalar load it is waited for where it is issued).
template <typename T> __device__ __forceinline__ T pinned(T v) { asm volatile("" : "+v"(v)); return v; }

// values that ARE wave-uniform but derive from cross-lane operations (which the compiler's divergence analysis cannot see through)
__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ const char *uniform_ptr(const char *q) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(q);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return reinterpret_cast<const char *>(((unsigned long long)hi << 32) | lo);
}

// ---- DPP moves.  dpp_i / dpp_f / dpp_d: out-of-range / masked lanes read 0 (old value 0, bound_ctrl on).
template <int CTRL, int ROW_MASK = 0xF> __device__ __forceinline__ int dpp_i(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xF, true); }
template <int CTRL, int ROW_MASK = 0xF> __device__ __forceinline__ float dpp_f(float x) {
    return __builtin_bit_cast(float, dpp_i<CTRL, ROW_MASK>(__builtin_bit_cast(int, x)));
}
template <int CTRL, int ROW_MASK = 0xF> __device__ __forceinline__ double dpp_d(double x) {
    const int lo = dpp_i<CTRL, ROW_MASK>(__double2loint(x)), hi = dpp_i<CTRL, ROW_MASK>(__double2hiint(x));
    return __hiloint2double(hi, lo);
}
// quad / row permutation of a double, every lane valid (old value = self, bound_ctrl off): NOT interchangeable with dpp_d
template <int CTRL> __device__ __forceinline__ double dpp_q(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// ---- lane reads
__device__ __forceinline__ float readlane_f(float x, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
}
__device__ __forceinline__ double readlane_d(double x, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

// ---- scans
// inclusive prefix sum over the 16 lanes of a row
__device__ __forceinline__ double row_scan(double x) {
    x += dpp_d<0x111>(x); // row_shr:1
    x += dpp_d<0x112>(x); // row_shr:2
    x += dpp_d<0x114>(x); // row_shr:4
    x += dpp_d<0x118>(x); // row_shr:8
    return x;
}
// inclusive prefix sum over the 64 lanes of a wavefront (lane 63 ends up with the wave total)
__device__ __forceinline__ double wave_scan(double x) {
    x = row_scan(x);
    x += dpp_d<0x142, 0xA>(x); // row_bcast:15 into rows 1 and 3
    x += dpp_d<0x143, 0xC>(x); // row_bcast:31 into rows 2 and 3
    return x;
}
__device__ __forceinline__ float wave_scan_f(float x) {
    x += dpp_f<0x111>(x);
    x += dpp_f<0x112>(x);
    x += dpp_f<0x114>(x);
    x += dpp_f<0x118>(x);
    x += dpp_f<0x142, 0xA>(x);
    x += dpp_f<0x143, 0xC>(x);
    return x;
}
// maximum of non-negative values over the wavefront, DPP only (no LDS round trips): a max-scan leaves it in lane 63; returned wave-uniform
__device__ __forceinline__ float wave_max_nonneg(float x) {
    x = fmaxf(x, dpp_f<0x111>(x));
    x = fmaxf(x, dpp_f<0x112>(x));
    x = fmaxf(x, dpp_f<0x114>(x));
    x = fmaxf(x, dpp_f<0x118>(x));
    x = fmaxf(x, dpp_f<0x142, 0xA>(x));
    x = fmaxf(x, dpp_f<0x143, 0xC>(x));
    return readlane_f(x, 63);
}

// ---- Totals of FOUR f64 values over the wavefront, every lane receiving all four -- a transpose-reduce instead of four scans: the first
// two steps trade values between lane pairs (lane ^ 1: even lanes keep a and c, odd lanes b and d; lane ^ 2: one value per lane,
// quantity = lane & 3), two row rotations add the four lanes of a row that hold the same quantity, and gfx950's
// v_permlane16_swap / v_permlane32_swap add the rows.  Eight 64-bit additions and 14 lane movements instead of 24 and 48.
__device__ __forceinline__ double rows_sum16(double x) { // [r0, r1, r2, r3] -> [r0 + r1, r0 + r1, r2 + r3, r2 + r3], lane for lane
    const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(x), __double2loint(x), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(x), __double2hiint(x), false, false);
    return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ double halves_sum32(double x) { // [lower, upper] -> lower + upper in both halves, lane for lane
    const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(x), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(x), false, false);
    return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ void wave_sum4(double &a, double &b, double &c, double &d, int lane) {
    const bool o1 = (lane & 1) != 0, o2 = (lane & 2) != 0;
    double k0 = o1 ? b : a, k1 = o1 ? d : c;            // kept; the partner receives the other two
    k0 += dpp_q<0xB1>(o1 ? a : b);                       // quad_perm [1,0,3,2]: lane ^ 1
    k1 += dpp_q<0xB1>(o1 ? c : d);
    double k = o2 ? k1 : k0;
    k += dpp_q<0x4E>(o2 ? k0 : k1);                      // quad_perm [2,3,0,1]: lane ^ 2 -> quantity (lane & 3) summed over the quad
    k += dpp_q<0x124>(k);                                // row_ror:4
    k += dpp_q<0x128>(k);                                // row_ror:8 -> ... over the row
    k = halves_sum32(rows_sum16(k));                     // ... over the wavefront
    a = readlane_d(k, 0); b = readlane_d(k, 1); c = readlane_d(k, 2); d = readlane_d(k, 3);
}

} // namespace ofdm
