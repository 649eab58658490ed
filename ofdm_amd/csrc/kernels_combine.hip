// kernels_combine.hip -- EXT-7 soft combining (ofdm_llr_combine_batch, the combine step of ofdm_rx_decode_combine_batch; definition:
// tests/combine_ref.py, include/ofdm_hip.h).
//
// A streaming kernel: the int8 LLR rows of a frame's R branches in, one combined row out.  The unit of work is (frame, chunk of kChunk
// LLRs); a WAVEFRONT owns a unit and the wavefronts of a persistent grid stride over the units, so no barrier and no LDS is needed and
// the bytes cannot depend on the grid.  Per unit:
//   1. lane r < R forms branch r's verdict (live?), its LLR unit u_r, its counted length n_r and -- after a three-step butterfly for
//      u_max -- its weight q_r = rint(64 u_r / u_max) in f64: one division a unit, wave-uniform per frame.  Every unit of a frame forms
//      the same values; the unit of chunk 0 alone writes them (q_r by the lane that formed it, status_f and nsym_f by lane 0): no
//      atomics, no zeroed counters, no second launch.
//   2. the branches that count in this chunk (q_r > 0 and n_r beyond the chunk's start) are compacted through a ballot into A <= 8
//      wave-uniform (row, q, n) triples, and the chunk runs through the instantiation for that A: a dead or zero-weight branch, or one
//      that ended in front of the chunk, costs nothing and is not read.
//   3. per tile of 1 KiB: where every row is 16-byte aligned and the tile lies inside every counting branch and inside n_llr, each lane
//      loads 16 bytes of each of the A rows (all A loads issued unconditionally, then used), transposes them across branches with
//      v_perm_b32 into dwords (L_0[j], L_1[j], L_2[j], L_3[j]) and forms sum q_r L_r[j] + 32 with v_dot4_i32_i8 against the packed
//      weights (q_r <= 64 fits a byte; branches 4 .. 7 are a second dot into the same accumulator), shifts, clamps, packs and stores 16
//      bytes.  Every other tile -- unaligned rows, the tail of the row, a tile a branch ends in -- goes byte by byte, lane i at columns
//      i, i + 64, ..., each branch read only below its n_r.  Every input byte is read once.
#include <float.h>

#include "../../include/ofdm_hip.h"
#include "kernels.hpp"

namespace ofdm {

static_assert(kCombineMaxBranches == OFDM_COMBINE_MAX_BRANCHES, "the bound of include/ofdm_hip.h");

namespace {
constexpr int kTile = 1024;          // 64 lanes x 16 bytes
constexpr int kChunk = 4 * kTile;    // LLRs per unit: the weights are formed once per 4 KiB of every branch
typedef unsigned u32;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int clamp127(int v) { return v < -127 ? -127 : (v > 127 ? 127 : v); }

// Four combined LLRs from the dwords x[0 .. A): columns j .. j + 3 of each counting branch.  v_perm_b32(hi, lo, sel): byte i of the
// result is byte sel_i of the eight bytes {hi, lo}, lo's being 0 .. 3.
template <int A> __device__ __forceinline__ u32 combine4(const u32 (&x)[8], const u32 (&w)[2]) {
    int s[4] = {32, 32, 32, 32};
#pragma unroll
    for (int g = 0; g < (A + 3) / 4; ++g) {
        const u32 a = x[4 * g], b = 4 * g + 1 < A ? x[4 * g + 1] : 0u, c = 4 * g + 2 < A ? x[4 * g + 2] : 0u, d = 4 * g + 3 < A ? x[4 * g + 3] : 0u;
        const u32 ab_lo = __builtin_amdgcn_perm(b, a, 0x05010400u), ab_hi = __builtin_amdgcn_perm(b, a, 0x07030602u); // a0 b0 a1 b1 | a2 b2 a3 b3
        const u32 cd_lo = __builtin_amdgcn_perm(d, c, 0x05010400u), cd_hi = __builtin_amdgcn_perm(d, c, 0x07030602u);
        s[0] = __builtin_amdgcn_sdot4((int)__builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u), (int)w[g], s[0], false);  // a0 b0 c0 d0
        s[1] = __builtin_amdgcn_sdot4((int)__builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u), (int)w[g], s[1], false);
        s[2] = __builtin_amdgcn_sdot4((int)__builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u), (int)w[g], s[2], false);
        s[3] = __builtin_amdgcn_sdot4((int)__builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u), (int)w[g], s[3], false);
    }
    u32 r = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) r |= (u32)(clamp127(s[i] >> 6) & 0xff) << (8 * i);
    return r;
}

// LLRs [j0, j1) of one frame from its A counting branches: row[k] read below n[k] only, with weight q[k]
template <int A>
__device__ __forceinline__ void combine_chunk(const int8_t *const (&row)[8], const int (&q)[8], const int (&n)[8], int8_t *out, int n_llr, int j0,
                                              int j1, bool vec, int lane) {
    u32 w[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < A; ++k) w[k >> 2] |= (u32)q[k] << (8 * (k & 3));
    for (int t0 = j0; t0 < j1; t0 += kTile) {
        const int t1 = t0 + kTile;
        bool whole = vec && t1 <= n_llr;
#pragma unroll
        for (int k = 0; k < A; ++k) whole = whole && t1 <= n[k];
        if (whole) {
            const int j = t0 + 16 * lane;
            u32x4 v[A > 0 ? A : 1];
#pragma unroll
            for (int k = 0; k < A; ++k) v[k] = *reinterpret_cast<const u32x4 *>(row[k] + j);
            u32x4 o;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                u32 x[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = k < A ? v[k][d] : 0u;
                o[d] = combine4<A>(x, w);
            }
            *reinterpret_cast<u32x4 *>(out + j) = o;
        } else {
            const int e = t1 < n_llr ? t1 : n_llr;
            for (int j = t0 + lane; j < e; j += 64) {
                int s = 32;
#pragma unroll
                for (int k = 0; k < A; ++k)
                    if (j < n[k]) s += q[k] * (int)row[k][j];
                out[j] = (int8_t)clamp127(s >> 6);
            }
        }
    }
}
} // namespace

__global__ __launch_bounds__(256) void k_llr_combine(CombineParams p) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * 4;
    const int R = p.n_branches, n_llr = p.n_llr;
    const long long per_row = n_llr > 0 ? ((long long)n_llr + kChunk - 1) / kChunk : 1; // (n_llr = 0: the weights still leave)
    const long long units = p.n_frames * per_row;
    const bool vec = ((reinterpret_cast<uintptr_t>(p.llr) | reinterpret_cast<uintptr_t>(p.out) | (uintptr_t)p.llr_stride | (uintptr_t)p.out_stride) & 15) == 0;
    for (long long unit = wave; unit < units; unit += n_waves) {
        const long long f = unit / per_row;
        const int c = (int)(unit - f * per_row);
        const int j0 = c * kChunk, j1 = n_llr - j0 < kChunk ? n_llr : j0 + kChunk;
        // ---- 1. lane r: branch r
        const bool mine = lane < R;
        const long long brow = f * R + (mine ? lane : 0);
        const int st = (mine && p.status) ? p.status[brow] : 0;
        bool live = mine && st == 0;
        float u = 1.f;
        if (mine && p.quality) {
            const float *qr = p.quality + brow * kQualityFields;
            u = qr[OFDM_Q_LLR_UNIT];
            live = live && qr[OFDM_Q_VALID] == 1.f && u > 0.f && u <= FLT_MAX; // finite and > 0 (NaN fails both)
        }
        const int raw = (mine && p.n_live) ? p.n_live[brow] : 0;
        long long nl = p.n_live ? (long long)raw * p.live_unit : (long long)n_llr;
        nl = !mine || nl < 0 ? 0 : (nl > n_llr ? n_llr : nl);
        float um = live ? u : 0.f;
#pragma unroll
        for (int s = 1; s <= 4; s <<= 1) um = fmaxf(um, __shfl_xor(um, s, 64)); // lanes 0 .. 7 hold the branches
        int q = 0;
        if (live) q = (int)__builtin_rint(64.0 * (double)u / (double)um);           // IEEE f64 quotient, ties to even
        if (c == 0) {
            if (mine && p.weight) p.weight[brow] = q;
            if (p.status_out) {
                const unsigned long long alive = __ballot(live), bad = __ballot(mine && st != 0);
                int ns = live ? raw : 0;
#pragma unroll
                for (int s = 1; s <= 4; s <<= 1) ns = max(ns, __shfl_xor(ns, s, 64));
                const int first_bad = __builtin_amdgcn_readlane(st, bad ? __ffsll((long long)bad) - 1 : 0);
                const int sf = alive ? OFDM_FRAME_OK : (bad ? first_bad : OFDM_FRAME_HEADER);
                if (lane == 0) { p.status_out[f] = sf; p.nsym_out[f] = ns; }
            }
        }
        // ---- 2. the branches that count in this chunk, compacted
        const int nli = (int)nl;
        u32 am = (u32)__ballot(q > 0 && nli > j0) & 0xffu;
        const int A = __popc(am);
        const int8_t *row[8];
        int qk[8], nk[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool on = am != 0;
            const int r = on ? __ffs((int)am) - 1 : 0;
            am &= am - 1;
            qk[k] = on ? __builtin_amdgcn_readlane(q, r) : 0;
            nk[k] = on ? __builtin_amdgcn_readlane(nli, r) : 0;
            row[k] = p.llr + (f * R + r) * p.llr_stride;
        }
        // ---- 3. the chunk
        int8_t *out = p.out + f * p.out_stride;
        switch (A) {
        case 0: combine_chunk<0>(row, qk, nk, out, n_llr, j0, j1, vec, lane); break; // nothing counts: zeros
        case 1: combine_chunk<1>(row, qk, nk, out, n_llr, j0, j1, vec, lane); break;
        case 2: combine_chunk<2>(row, qk, nk, out, n_llr, j0, j1, vec, lane); break;
        case 3: combine_chunk<3>(row, qk, nk, out, n_llr, j0, j1, vec, lane); break;
        case 4: combine_chunk<4>(row, qk, nk, out, n_llr, j0, j1, vec, lane); break;
        case 5: combine_chunk<5>(row, qk, nk, out, n_llr, j0, j1, vec, lane); break;
        case 6: combine_chunk<6>(row, qk, nk, out, n_llr, j0, j1, vec, lane); break;
        case 7: combine_chunk<7>(row, qk, nk, out, n_llr, j0, j1, vec, lane); break;
        default: combine_chunk<8>(row, qk, nk, out, n_llr, j0, j1, vec, lane); break;
        }
    }
}

hipError_t run_llr_combine(const CombineParams &p, int num_cu, hipStream_t st) {
    if (p.n_frames <= 0) return hipSuccess;
    const long long per_row = p.n_llr > 0 ? ((long long)p.n_llr + kChunk - 1) / kChunk : 1;
    const long long units = p.n_frames * per_row;
    // persistent: 8 workgroups of four wavefronts per CU, one unit per wavefront and step
    const unsigned grid = (unsigned)persistent_grid((units + 3) / 4, (long long)num_cu * 8, tuning_or_default(p.tune));
    trace_add(p.trace, "k_llr_combine");
    hipLaunchKernelGGL(k_llr_combine, dim3(grid), dim3(256), 0, st, p);
    return hipGetLastError();
}

} // namespace ofdm
