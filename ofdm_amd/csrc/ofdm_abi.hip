// ofdm_abi.hip -- the extern "C" boundary of libofdm_hip.so (include/ofdm_hip.h).
// Context, parameter validation, host-side constant tables (f64 -> f32), workspace and the orchestration of
// the TX / RX pipelines.  No exceptions cross the boundary; every HIP failure is mapped to OFDM_ERR_HIP.
#include "ofdm_ctx.hpp"
#include "ldpc_table.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

namespace ofdm {
int sc_tile_lags();
}
using namespace ofdm;

namespace {

constexpr double kPi = 3.14159265358979323846;

struct cd { double re, im; };
static inline cd cd_mul(cd a, cd b) { return cd{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

// host f64 radix-2 FFT for the constant tables (product code: independent of oracle/)
static void host_fft(std::vector<cd> &x, bool inverse) {
    const size_t n = x.size();
    for (size_t i = 1, j = 0; i < n; i++) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(x[i], x[j]);
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        for (size_t k = 0; k < len / 2; k++) {
            double ang = (inverse ? 2.0 : -2.0) * kPi * (double)k / (double)len;
            cd w{std::cos(ang), std::sin(ang)};
            for (size_t i = k; i < n; i += len) {
                cd u = x[i], v = cd_mul(x[i + len / 2], w);
                x[i] = cd{u.re + v.re, u.im + v.im};
                x[i + len / 2] = cd{u.re - v.re, u.im - v.im};
            }
        }
    }
    if (inverse)
        for (auto &v : x) { v.re /= (double)n; v.im /= (double)n; }
}

static uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static double uniform_pm1(uint64_t &s) { return (double)(splitmix64(s) >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0; }

static bool valid_nfft(int n) { return n >= 64 && n <= 4096 && (n & (n - 1)) == 0; }

} // namespace

static SymParams base_params(ofdm_ctx *c) {
    SymParams p;
    p.tune = &c->tune;
    p.trace = &c->trace;
    p.tw = c->d_tw;
    p.inv_training = c->d_inv_trn;
    p.sym_len = c->S();
    p.bps = c->prm.modulation;
    p.guard = c->prm.guard_bands;
    return p;
}
// ... of a receive stream: n_frames captures of frame_len samples, frame_stride apart, each with its own (optional) trimmed start,
// CFO and live-symbol count; out_bytes / out_stride: the per-frame rows of demodulated bytes (none for the channel estimate)
static SymParams rx_params(ofdm_ctx *c, const float2 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len, const int32_t *offset,
                           const double *f_delta, const int32_t *nsym_frame = nullptr, uint8_t *out_bytes = nullptr, int64_t out_stride = 0) {
    SymParams p = base_params(c);
    p.in = in; p.n_frames = n_frames; p.frame_stride = frame_stride; p.frame_len = frame_len;
    p.offset = offset; p.f_delta = f_delta; p.nsym_frame = nsym_frame;
    p.out_bytes = out_bytes; p.out_stride = out_stride;
    return p;
}

// What one shape-specialised path made of a call: OFDM_OK = it took it, OFDM_ERR_HIP = it failed (code in last_hip), kNextPath = it
// declined (hipErrorNotSupported: outside its envelope, or switched off by its A/B tuning key) and the next path in line is tried.
static const int kNextPath = 1;
static int fast_path(ofdm_ctx *c, hipError_t e) {
    if (e == hipSuccess) return OFDM_OK;
    if (e == hipErrorNotSupported) return kNextPath;
    c->last_hip = (int)e;
    return OFDM_ERR_HIP;
}
#define FAST_PATH(ctx, off, call)                                                          \
    do {                                                                                   \
        const int _r = fast_path(ctx, (off) ? hipErrorNotSupported : (call));              \
        if (_r != kNextPath) return _r;                                                    \
    } while (0)

// ---- EXT-5 channel-estimate denoising: host side (include/ofdm_hip.h, tests/chest_ref.py)
// R^-1 of the Hermitian Toeplitz R[n][m] = r[n - m], r[d] = sum_k |t_k|^2 e^{+2 pi i k d / N}, L = N / 4, in f64 by Trench's algorithm:
// the Levinson recursion gives x = the first column of R^-1 in O(L^2), and the Gohberg-Semencul identity fills the rest,
//   B[i + 1][j + 1] = B[i][j] + (x[i + 1] conj(x[j + 1]) - conj(x[L - 1 - i]) x[L - 1 - j]) / x[0].
// The recursion runs along diagonals from the first row and column only as far as the anti-diagonal; the other half follows from
// persymmetry, B[i][j] = B[L - 1 - j][L - 1 - i], so no entry is more than L / 2 additions away from x.
// false when R is not positive definite (fewer than L non-zero training bins), or when what came out is not its inverse (below).
static const double kChestResidual = 1e-6;
static bool chest_rinv(int N, const double *trn, std::vector<cd> &B) {
    const int L = N / 4;
    std::vector<cd> r(N);
    for (int k = 0; k < N; k++) r[k] = cd{trn[2 * k] * trn[2 * k] + trn[2 * k + 1] * trn[2 * k + 1], 0.0};
    host_fft(r, true);
    for (auto &v : r) { v.re *= (double)N; v.im *= (double)N; }
    if (!(r[0].re > 0.0)) return false;
    std::vector<cd> x(L, cd{0.0, 0.0}), nx(L);
    x[0] = cd{1.0 / r[0].re, 0.0};
    for (int m = 1; m < L; m++) { // x solves the leading m x m system R x = e_0; extend to m + 1
        cd eps{0.0, 0.0};
        for (int i = 0; i < m; i++) { const cd t = cd_mul(r[m - i], x[i]); eps.re += t.re; eps.im += t.im; }
        const double den = 1.0 - (eps.re * eps.re + eps.im * eps.im);
        if (!(den > 0.0)) return false;
        for (int i = 0; i <= m; i++) {
            const cd f = i < m ? x[i] : cd{0.0, 0.0};
            const cd b = i > 0 ? cd{x[m - i].re, -x[m - i].im} : cd{0.0, 0.0};
            const cd eb = cd_mul(eps, b);
            nx[i] = cd{(f.re - eb.re) / den, (f.im - eb.im) / den};
        }
        for (int i = 0; i <= m; i++) x[i] = nx[i];
    }
    const double x0 = x[0].re;
    if (!(x0 > 0.0)) return false;
    B.assign((size_t)L * L, cd{0.0, 0.0});
    for (int i = 0; i < L; i++)
        for (int j = 0; i + j < L; j++) {
            cd v;
            if (j == 0) v = x[i];
            else if (i == 0) v = cd{x[j].re, -x[j].im};
            else {
                const cd a = cd_mul(x[i], cd{x[j].re, -x[j].im});
                const cd b = cd_mul(cd{x[L - i].re, -x[L - i].im}, x[L - j]);
                const cd p = B[(size_t)(i - 1) * L + (j - 1)];
                v = cd{p.re + (a.re - b.re) / x0, p.im + (a.im - b.im) / x0};
            }
            B[(size_t)i * L + j] = v;
            B[(size_t)(L - 1 - j) * L + (L - 1 - i)] = v;
        }
    // The recursion only fails outright when a pivot turns non-positive.  A table that is zero on a whole band (guard bands nulled) makes
    // R singular to rounding, and the recursion may then run to its end on pivots that are rounding residue: B is verified as an inverse,
    // |R B - I| <= kChestResidual on at most 64 evenly spaced columns (all of them up to N = 256), and refused otherwise.  The device keeps
    // the table in f32, so a residual beyond that is no usable table.
    const int step = L > 64 ? L / 64 : 1;
    std::vector<cd> col(L);
    for (int j = 0; j < L; j += step) {
        for (int m = 0; m < L; m++) col[m] = B[(size_t)m * L + j];
        for (int i = 0; i < L; i++) {
            cd s{i == j ? -1.0 : 0.0, 0.0};
            const cd *ri = r.data() + i; // R[i][m] = r[i - m], taken mod N
            for (int m = 0; m <= i; m++) { const cd t = cd_mul(ri[-m], col[m]); s.re += t.re; s.im += t.im; }
            for (int m = i + 1; m < L; m++) { const cd t = cd_mul(ri[N - m], col[m]); s.re += t.re; s.im += t.im; }
            if (!(s.re * s.re + s.im * s.im <= kChestResidual * kChestResidual)) return false;
        }
    }
    return true;
}

// the device tables of the stage, built once per context
static int chest_tables(ofdm_ctx *c) {
    if (c->d_chest_mt) return OFDM_OK;
    const int N = c->prm.n_fft, L = N / 4;
    std::vector<cd> B;
    if (!chest_rinv(N, c->training.data(), B)) return OFDM_ERR_INVALID;
    std::vector<float> w(N);
    std::vector<float2> mt((size_t)L * L);
    for (int k = 0; k < N; k++) { const double re = c->training[2 * k], im = c->training[2 * k + 1]; w[k] = (float)(re * re + im * im); }
    for (int m = 0; m < L; m++) // the inverse FFT in front of the solve carries 1 / N: the table carries the N (a power of two: exact)
        for (int n = 0; n < L; n++) mt[(size_t)n * L + m] = make_float2((float)(B[(size_t)m * L + n].re * N), (float)(B[(size_t)m * L + n].im * N));
    float *dw = nullptr;
    float2 *dm = nullptr;
    if (hipMalloc(&dw, sizeof(float) * N) != hipSuccess) return OFDM_ERR_NOMEM;
    if (hipMalloc(&dm, sizeof(float2) * mt.size()) != hipSuccess) { hipFree(dw); return OFDM_ERR_NOMEM; }
    if (hipMemcpy(dw, w.data(), sizeof(float) * N, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dm, mt.data(), sizeof(float2) * mt.size(), hipMemcpyHostToDevice) != hipSuccess) { hipFree(dw); hipFree(dm); return OFDM_ERR_HIP; }
    c->d_chest_w = dw;
    c->d_chest_mt = dm;
    return OFDM_OK;
}

// ---- EXT-8 wide CFO acquisition: the training table t_k on the device (d_inv_trn holds 1 / t_k, k_cfo_wide matches against conj(t_k))
static int cfo_wide_table(ofdm_ctx *c) {
    if (c->d_trn) return OFDM_OK;
    const int N = c->prm.n_fft;
    std::vector<float2> t(N);
    for (int k = 0; k < N; k++) t[k] = make_float2((float)c->training[2 * k], (float)c->training[2 * k + 1]);
    float2 *dt = nullptr;
    if (hipMalloc(&dt, sizeof(float2) * N) != hipSuccess) return OFDM_ERR_NOMEM;
    if (hipMemcpy(dt, t.data(), sizeof(float2) * N, hipMemcpyHostToDevice) != hipSuccess) { hipFree(dt); return OFDM_ERR_HIP; }
    c->d_trn = dt;
    return OFDM_OK;
}

// rows of N bins `in` -> `out` (in == out allowed), per frame chunk: weight -> inverse FFT -> k_chest_solve -> forward FFT.  The
// one workspace (the solve's zeroed rows) holds a chunk, at most kChestChunkBytes whatever n_frames is.
static const int64_t kChestChunkBytes = 64ll << 20;
static int chest_smooth_run(ofdm_ctx *c, const float2 *in, int64_t n_frames, float2 *out) {
    int rc = chest_tables(c);
    if (rc) return rc;
    const int N = c->prm.n_fft;
    int64_t chunk = std::max<int64_t>(kChestChunkBytes / ((int64_t)sizeof(float2) * N), 64);
    if (chunk > n_frames) chunk = n_frames;
    void *w_taps;
    if ((rc = ws_get(c, kWsChestTaps, sizeof(float2) * (size_t)N * (size_t)chunk, &w_taps))) return rc;
    for (int64_t f0 = 0; f0 < n_frames; f0 += chunk) {
        const int64_t nf = n_frames - f0 < chunk ? n_frames - f0 : chunk;
        const Trace::Mute later(c->trace, f0 > 0); // the dispatch string names what a chunk ran, once
        float2 *rows = out + f0 * N;
        if (c->tune.chest_solve_only) { // laboratory key: the contraction alone, timed by tools/bench_chest.py
            ChestSolveParams sp;
            sp.g = in + f0 * N; sp.out = (float2 *)w_taps; sp.mt = c->d_chest_mt; sp.n_frames = nf; sp.n_fft = N; sp.n_taps = N / 4; sp.pre = N / 16;
            c->trace.add("k_chest_solve");
            HIP_TRY(c, run_chest_solve(sp, c->num_cu, &c->tune, c->stream));
            continue;
        }
        c->trace.add("k_chest_weight");
        HIP_TRY(c, run_chest_weight(in + f0 * N, c->d_chest_w, rows, nf, N, c->num_cu, &c->tune, c->stream));
        SymParams p = base_params(c);
        p.n_frames = nf; p.frame_stride = N; p.frame_len = N; p.syms_per_frame = 1; p.in_sym_stride = N; p.in_skip = 0;
        p.in = rows; p.out = rows;
        HIP_TRY(c, run_fft(N, p, true, c->stream, c->num_cu));
        ChestSolveParams sp;
        sp.g = rows; sp.out = (float2 *)w_taps; sp.mt = c->d_chest_mt; sp.n_frames = nf; sp.n_fft = N; sp.n_taps = N / 4; sp.pre = N / 16;
        c->trace.add("k_chest_solve");
        HIP_TRY(c, run_chest_solve(sp, c->num_cu, &c->tune, c->stream));
        p.in = (const float2 *)w_taps; p.out = rows;
        HIP_TRY(c, run_fft(N, p, false, c->stream, c->num_cu));
    }
    return OFDM_OK;
}

extern "C" {

int ofdm_abi_version(void) { return OFDM_HIP_ABI_VERSION; }

const char *ofdm_strerror(int status) {
    switch (status) {
    case OFDM_OK: return "ok";
    case OFDM_ERR_INVALID: return "invalid argument";
    case OFDM_ERR_UNSUPPORTED: return "unsupported configuration";
    case OFDM_ERR_NO_DEVICE: return "no usable HIP device";
    case OFDM_ERR_HIP: return "HIP runtime error";
    case OFDM_ERR_NOMEM: return "out of device memory";
    case OFDM_ERR_UNCORRECTABLE: return "uncorrectable Reed-Solomon block";
    default: return "unknown status";
    }
}

int ofdm_device_count(int *count) {
    if (!count) return OFDM_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return OFDM_ERR_NO_DEVICE; }
    *count = n;
    return OFDM_OK;
}

int ofdm_default_params(ofdm_params *p) {
    if (!p) return OFDM_ERR_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->n_fft = 64;           // src/transmitter.rs:33,52
    p->cp_len = 16;
    p->modulation = OFDM_MOD_BPSK; // transmitter.rs:17
    p->guard_bands = 0;            // transmitter.rs:16
    p->ecc = OFDM_ECC_NONE;
    p->sync_window_reps = 3;
    p->sync_backoff = 4;
    p->cfo_mode = OFDM_CFO_SIGNED;
    p->sync_threshold = 0.5f;
    return OFDM_OK;
}

int ofdm_default_pilots(int32_t n_fft, int32_t cp_len, double *preamble, double *training) {
    if (!valid_nfft(n_fft) || cp_len != n_fft / 4) return OFDM_ERR_INVALID;
    if (preamble) {
        uint64_t s = 100; // transmitter.rs:76
        for (int i = 0; i < n_fft + cp_len; i++) {
            double re = uniform_pm1(s), im = uniform_pm1(s);
            preamble[2 * i] = re * 0.25;
            preamble[2 * i + 1] = im * 0.25;
        }
    }
    if (training) {
        uint64_t s = 50; // transmitter.rs:89
        for (int i = 0; i < n_fft; i++) {
            double re = uniform_pm1(s), im = uniform_pm1(s);
            training[2 * i] = re * 1.0;
            training[2 * i + 1] = im * 1.0;
        }
    }
    return OFDM_OK;
}

// ---- rand 0.8 `StdRng` (= ChaCha12Rng of rand_chacha 0.3) restated from the crates' published algorithm, for the
// reference's pilot tables (src/transmitter.rs:75-96).  The ChaCha core is pinned by the published RFC 7539 / ChaCha12
// test vectors (tests/test_abi_cpu.py); seeding (rand_core 0.6 seed_from_u64: PCG32 expansion) and the f64
// gen_range(-1.0..1.0) mapping (rand 0.8.3 UniformFloat::sample_single: 52 mantissa bits -> [1,2) - 1, * scale + low)
// cannot be checked against a running `rand` here: the tables are "unverified" (DESIGN.md section 2).
namespace {
struct StdRng {
    uint32_t key[8];
    uint64_t counter = 0;
    uint32_t buf[16];
    int idx = 16;
    static uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
    static void qr(uint32_t *s, int a, int b, int c, int d) {
        s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 16);
        s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 12);
        s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 8);
        s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 7);
    }
    static void block(const uint32_t key[8], const uint32_t w12_15[4], int rounds, uint32_t out[16]) {
        uint32_t st[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
        for (int i = 0; i < 8; i++) st[4 + i] = key[i];
        for (int i = 0; i < 4; i++) st[12 + i] = w12_15[i];
        uint32_t s[16];
        for (int i = 0; i < 16; i++) s[i] = st[i];
        for (int r = 0; r < rounds / 2; r++) {
            qr(s, 0, 4, 8, 12); qr(s, 1, 5, 9, 13); qr(s, 2, 6, 10, 14); qr(s, 3, 7, 11, 15);
            qr(s, 0, 5, 10, 15); qr(s, 1, 6, 11, 12); qr(s, 2, 7, 8, 13); qr(s, 3, 4, 9, 14);
        }
        for (int i = 0; i < 16; i++) out[i] = s[i] + st[i];
    }
    explicit StdRng(uint64_t state) { // SeedableRng::seed_from_u64: PCG32 output per 4 seed bytes (little endian)
        for (int i = 0; i < 8; i++) {
            state = state * 6364136223846793005ull + 11634580027462260723ull;
            const uint32_t xorshifted = (uint32_t)(((state >> 18) ^ state) >> 27);
            const uint32_t rot = (uint32_t)(state >> 59);
            key[i] = (xorshifted >> rot) | (xorshifted << ((32 - rot) & 31));
        }
    }
    uint32_t next_u32() {
        if (idx == 16) { // 64-bit block counter in words 12-13, stream id 0 in words 14-15
            const uint32_t w[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), 0u, 0u};
            block(key, w, 12, buf);
            ++counter;
            idx = 0;
        }
        return buf[idx++];
    }
    uint64_t next_u64() { const uint64_t lo = next_u32(); return lo | ((uint64_t)next_u32() << 32); } // BlockRng: low word first
    double range_pm1() { // gen_range(-1.0..1.0)
        const uint64_t bits = (next_u64() >> 12) | 0x3ff0000000000000ull;
        double v;
        std::memcpy(&v, &bits, 8);
        return (v - 1.0) * 2.0 + -1.0;
    }
};
} // namespace

int ofdm_stdrng_pilots(int32_t n_fft, int32_t cp_len, double *preamble, double *training) {
    if (!valid_nfft(n_fft) || cp_len != n_fft / 4) return OFDM_ERR_INVALID;
    if (preamble) {
        StdRng r(100); // transmitter.rs:76
        for (int i = 0; i < n_fft + cp_len; i++) {
            const double re = r.range_pm1(), im = r.range_pm1(); // re drawn before im (transmitter.rs:80)
            preamble[2 * i] = re * 0.25;
            preamble[2 * i + 1] = im * 0.25;
        }
    }
    if (training) {
        StdRng r(50); // transmitter.rs:89
        for (int i = 0; i < n_fft; i++) {
            const double re = r.range_pm1(), im = r.range_pm1();
            training[2 * i] = re;
            training[2 * i + 1] = im;
        }
    }
    return OFDM_OK;
}

uint32_t ofdm_crc32(const uint8_t *data, int64_t n_bytes) { return (!data || n_bytes < 0) ? 0u : crc32_host(data, n_bytes); }

int ofdm_chacha_block(const uint32_t *key8, const uint32_t *words12_15, int32_t rounds, uint32_t *out16) {
    if (!key8 || !words12_15 || !out16 || rounds <= 0 || (rounds & 1)) return OFDM_ERR_INVALID;
    StdRng::block(key8, words12_15, rounds, out16);
    return OFDM_OK;
}

int ofdm_destroy(ofdm_ctx *c) {
    if (!c) return OFDM_OK;
    int prev_dev = -1;
    const bool have_prev = hipGetDevice(&prev_dev) == hipSuccess;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    ofdm_host_pipe_destroy(c);
    for (auto &w : c->ws) if (w.ptr) hipFree(w.ptr);
    if (c->d_tw) hipFree(c->d_tw);
    if (c->d_inv_trn) hipFree(c->d_inv_trn);
    if (c->d_header) hipFree(c->d_header);
    if (c->d_chest_w) hipFree(c->d_chest_w);
    if (c->d_chest_mt) hipFree(c->d_chest_mt);
    if (c->d_trn) hipFree(c->d_trn);
    if (c->d_stats) hipFree(c->d_stats);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;
    if (have_prev) hipSetDevice(prev_dev);
    return OFDM_OK;
}

int ofdm_create(const ofdm_params *p, const double *preamble, const double *training, int device, void *stream,
                ofdm_ctx **out) {
    if (!p || !out) return OFDM_ERR_INVALID;
    *out = nullptr;
    if (!valid_nfft(p->n_fft) || p->cp_len != p->n_fft / 4) return OFDM_ERR_INVALID;
    switch (p->modulation) {
    case OFDM_MOD_BPSK: case OFDM_MOD_QPSK: case OFDM_MOD_QAM16: case OFDM_MOD_QAM64: case OFDM_MOD_QAM256: break;
    default: return OFDM_ERR_INVALID;
    }
    if (p->guard_bands != 0 && p->guard_bands != 1) return OFDM_ERR_INVALID;
    ModePlan mode;
    if (!mode_plan(p->ecc, &mode)) return OFDM_ERR_INVALID;
    if (p->sync_window_reps < 1 || p->sync_window_reps > 3) return OFDM_ERR_INVALID;
    if (p->sync_backoff < 0 || p->sync_backoff > p->cp_len) return OFDM_ERR_INVALID;
    if (p->cfo_mode < OFDM_CFO_OFF || p->cfo_mode > OFDM_CFO_WIDE) return OFDM_ERR_INVALID;
    if (!(p->sync_threshold > 0.f && p->sync_threshold <= 1.f)) return OFDM_ERR_INVALID;
    if (p->sync_mode != OFDM_SYNC_SCHMIDL_COX && p->sync_mode != OFDM_SYNC_REFERENCE) return OFDM_ERR_INVALID;
    if (p->cfo_mode == OFDM_CFO_WIDE && p->sync_mode != OFDM_SYNC_SCHMIDL_COX) return OFDM_ERR_INVALID; // the hypotheses refine the Schmidl-Cox phase
    if (p->rx_path != OFDM_RX_AUTO && p->rx_path != OFDM_RX_STAGED) return OFDM_ERR_INVALID; // (2 was the one-pass kernel of rounds 2-4: removed)
    if (p->chest_mode != OFDM_CHEST_LS && p->chest_mode != OFDM_CHEST_WLS) return OFDM_ERR_INVALID;
    // EXT-5 / EXT-8 model the channel's taps at delays [-cp/4, 3 cp/4) behind the frame start; a Schmidl-Cox frame start is
    // sync_backoff samples early, so the first tap sits at delay sync_backoff: at 3 cp/4 or more even a one-tap channel is outside
    if (p->sync_mode == OFDM_SYNC_SCHMIDL_COX && (p->chest_mode == OFDM_CHEST_WLS || p->cfo_mode == OFDM_CFO_WIDE) &&
        p->sync_backoff >= p->cp_len - p->cp_len / 4) return OFDM_ERR_INVALID;
    for (int r : p->reserved) if (r != 0) return OFDM_ERR_INVALID;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return OFDM_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return OFDM_ERR_NO_DEVICE;
    DeviceGuard dev_guard(device); // the caller's current device is restored on every return path
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return OFDM_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return OFDM_ERR_NO_DEVICE; // gfx950 code objects only

    ofdm_ctx *c = new (std::nothrow) ofdm_ctx();
    if (!c) return OFDM_ERR_NOMEM;
    c->prm = *p;
    c->mode = mode;
    c->device = device;
    c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    int rc = OFDM_OK;
    do {
        c->stream = (hipStream_t)stream; // NULL = the device's default (null) stream

        if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) { rc = OFDM_ERR_HIP; break; }

        const int N = p->n_fft, CP = p->cp_len, S = N + CP;
        std::vector<double> pre(2 * S), trn(2 * N);
        ofdm_default_pilots(N, CP, pre.data(), trn.data());
        if (preamble) std::memcpy(pre.data(), preamble, sizeof(double) * 2 * S);
        if (training) std::memcpy(trn.data(), training, sizeof(double) * 2 * N);
        c->training = trn;

        std::vector<float2> tw(N), inv(N), hdr(10 * S);
        for (int m = 0; m < N; m++) {
            double a = -2.0 * kPi * (double)m / (double)N;
            tw[m] = make_float2((float)std::cos(a), (float)std::sin(a));
            double re = trn[2 * m], im = trn[2 * m + 1], ns = re * re + im * im;
            inv[m] = make_float2((float)(re / ns), (float)(-im / ns));
        }
        // header = [locking_signal(S)] [preamble x4] [prefix_block(training) x5]  (src/transmitter.rs:22-34)
        std::vector<cd> lock(S);
        for (int i = 0; i < S; i++) lock[i] = cd{0.5 * ((double)i / (2.0 * (double)S) + 0.5), 0.0}; // transmitter.rs:63-66
        const int mid = (S + 1) / 2;                                                               // fft_shift, mod.rs:65
        for (int i = 0; i < S; i++) { cd v = lock[(i + mid) % S]; hdr[i] = make_float2((float)v.re, (float)v.im); }
        for (int r = 0; r < 4; r++)
            for (int i = 0; i < S; i++) hdr[(1 + r) * S + i] = make_float2((float)pre[2 * i], (float)pre[2 * i + 1]);
        std::vector<cd> t(N);
        for (int i = 0; i < N; i++) t[i] = cd{trn[2 * i], trn[2 * i + 1]};
        host_fft(t, true);
        for (int r = 0; r < 5; r++) {
            float2 *blk = hdr.data() + (5 + r) * S;
            for (int i = 0; i < CP; i++) blk[i] = make_float2((float)t[N - CP + i].re, (float)t[N - CP + i].im);
            for (int i = 0; i < N; i++) blk[CP + i] = make_float2((float)t[i].re, (float)t[i].im);
        }
        float hmax = 0.f;
        for (auto &v : hdr) { hmax = std::fmax(hmax, v.x); hmax = std::fmax(hmax, v.y); }
        c->header_max = hmax;

        if (hipMalloc(&c->d_tw, sizeof(float2) * N) != hipSuccess || hipMalloc(&c->d_inv_trn, sizeof(float2) * N) != hipSuccess ||
            hipMalloc(&c->d_header, sizeof(float2) * 10 * S) != hipSuccess ||
            hipMalloc(&c->d_stats, 2 * sizeof(int32_t)) != hipSuccess) { rc = OFDM_ERR_NOMEM; break; }
        if (hipMemcpy(c->d_tw, tw.data(), sizeof(float2) * N, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(c->d_inv_trn, inv.data(), sizeof(float2) * N, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(c->d_header, hdr.data(), sizeof(float2) * 10 * S, hipMemcpyHostToDevice) != hipSuccess) { rc = OFDM_ERR_HIP; break; }
        if (p->chest_mode == OFDM_CHEST_WLS) rc = chest_tables(c); // the host solve (its time per N)
        if (rc == OFDM_OK && p->cfo_mode == OFDM_CFO_WIDE) rc = cfo_wide_table(c);
    } while (0);
    if (rc != OFDM_OK) { ofdm_destroy(c); return rc; }
    *out = c;
    return OFDM_OK;
}

int ofdm_set_stream(ofdm_ctx *c, void *stream) {
    if (!c) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    if (c->own_stream && c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); c->own_stream = false; }
    c->stream = (hipStream_t)stream;
    return OFDM_OK;
}
int ofdm_use_own_stream(ofdm_ctx *c) {
    if (!c) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    if (c->own_stream) return OFDM_OK;
    hipStream_t s = nullptr;
    HIP_TRY(c, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (c->stream) hipStreamSynchronize(c->stream);
    c->stream = s;
    c->own_stream = true;
    return OFDM_OK;
}
int ofdm_synchronize(ofdm_ctx *c) {
    if (!c) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return OFDM_OK;
}
int ofdm_last_hip_error(const ofdm_ctx *c) { return c ? c->last_hip : 0; }

namespace {
struct TuneKey { const char *name; int Tuning::*field; bool profile_only; };
const TuneKey kTuneKeys[] = { // the laboratory keys: ofdm_hip_tuning.h (private); the public ones are handled by name below
#define OFDM_TUNE_KEY(name, field, prof) {name, &Tuning::field, prof},
#include "ofdm_hip_tuning.h"
#undef OFDM_TUNE_KEY
};
} // namespace

int ofdm_set_tuning(ofdm_ctx *c, const char *key, int64_t value) {
    if (!c || !key) return OFDM_ERR_INVALID;
    if (std::strcmp(key, "grid_cap") == 0) { if (value < 0) return OFDM_ERR_INVALID; c->tune.grid_cap = value; return OFDM_OK; }
    if (std::strcmp(key, "sync_threshold_bits") == 0) { // the threshold as the bit pattern of a double (ofdm_hip_tuning.h); 0 = the params' float again
        double thr;
        std::memcpy(&thr, &value, sizeof(thr));
        if (value != 0 && !(thr > 0.0 && thr <= 1.0)) return OFDM_ERR_INVALID;
        c->sync_threshold_f64 = thr;
        return OFDM_OK;
    }
    if (std::strcmp(key, "ws_poison") == 0) { // 0 = off, 0x100 + b = fill what is held now, and every later growth, with byte b (ofdm_hip_tuning.h)
        if (value != 0 && (value < 0x100 || value > 0x1FF)) return OFDM_ERR_INVALID;
        if (!value) { c->ws_poison = 0; return OFDM_OK; }
        DeviceGuard dev_guard(c->device);
        const int fill = (int)value & 0xFF;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (const Workspace &w : c->ws)
            if (w.ptr) { const int rc = poison_fill_dev(c, w.ptr, w.cap, fill); if (rc) return rc; }
        const int rc = ofdm_host_pipe_poison(c, fill);
        if (rc) return rc;
        c->ws_poison = (int)value; // on only when everything the context holds was filled: a failed arming leaves the key as it was
        return OFDM_OK;
    }
    for (const TuneKey &k : kTuneKeys)
        if (std::strcmp(key, k.name) == 0) {
            if (k.profile_only && !kProfile) return OFDM_ERR_UNSUPPORTED; // the ablation branches are not in this build
            if (value < 0 || value > 0x7fffffff) return OFDM_ERR_INVALID;
            // keys that size LDS tiles or pick template instantiations take only the values their kernels were built for
            if (k.field == &Tuning::sc_first_lags && value > 1280) return OFDM_ERR_INVALID;       // the first launch's 128-chunk tile holds 1280 samples
            if (k.field == &Tuning::tx_waves && (value < 1 || value > 32)) return OFDM_ERR_INVALID;
            if (k.field == &Tuning::demod64_burst && value != 16 && value != 8 && value != 4 && value != 1) return OFDM_ERR_INVALID;
            if (k.field == &Tuning::sc_wg_per_cu && value > 16) return OFDM_ERR_INVALID;
            c->tune.*(k.field) = (int)value;
            return OFDM_OK;
        }
    return OFDM_ERR_INVALID;
}
int ofdm_get_tuning(const ofdm_ctx *c, const char *key, int64_t *value) {
    if (!c || !key || !value) return OFDM_ERR_INVALID;
    if (std::strcmp(key, "grid_cap") == 0) { *value = c->tune.grid_cap; return OFDM_OK; }
    if (std::strcmp(key, "profile_build") == 0) { *value = kProfile ? 1 : 0; return OFDM_OK; }
    if (std::strcmp(key, "sync_threshold_bits") == 0) { std::memcpy(value, &c->sync_threshold_f64, sizeof(*value)); return OFDM_OK; }
    if (std::strcmp(key, "stat_sc_slow_frames") == 0 || std::strcmp(key, "stat_sc_redo_frames") == 0) {
        // counters of the LAST Schmidl-Cox search of this context (synchronises its stream); -1 when that search kept no such list
        const bool slow = key[8] == 's';
        *value = -1;
        if (!c->sc_stats.dev || !(slow ? c->sc_stats.has_slow : c->sc_stats.has_redo)) return OFDM_OK;
        const int32_t *src = c->sc_stats.dev + (slow ? 0 : 1);
        DeviceGuard dev_guard(c->device);
        int32_t v = 0;
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&v, src, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return OFDM_ERR_HIP;
        *value = v;
        return OFDM_OK;
    }
    if (std::strcmp(key, "ws_poison") == 0) { *value = c->ws_poison; return OFDM_OK; }
    if (std::strcmp(key, "stat_ws_roles") == 0) { *value = kWsRoles; return OFDM_OK; }
    if (std::strcmp(key, "stat_ws_live") == 0) { // bit r: role r holds memory
        static_assert(kWsRoles < 63, "stat_ws_live is one int64");
        *value = 0;
        for (int r = 0; r < kWsRoles; r++) if (c->ws[r].ptr) *value |= (int64_t)1 << r;
        return OFDM_OK;
    }
    if (std::strncmp(key, "stat_ws_ptr:", 12) == 0 || std::strncmp(key, "stat_ws_cap:", 12) == 0) { // role r's address / capacity
        char *end = nullptr;
        if (key[12] < '0' || key[12] > '9') return OFDM_ERR_INVALID; // digits only: no blank, no sign
        const long r = std::strtol(key + 12, &end, 10);
        if (*end || r >= kWsRoles) return OFDM_ERR_INVALID;
        *value = key[8] == 'p' ? (int64_t)(uintptr_t)c->ws[r].ptr : (int64_t)c->ws[r].cap;
        return OFDM_OK;
    }
    if (std::strcmp(key, "stat_pipe_bufs") == 0 || std::strncmp(key, "stat_pipe_ptr:", 14) == 0 || std::strncmp(key, "stat_pipe_cap:", 14) == 0 ||
        std::strncmp(key, "stat_pipe_pinned:", 17) == 0) { // the host pipe's buffers, as stat_ws_* shows the roles
        void *p = nullptr; size_t cap = 0; int pinned = 0;
        if (key[10] == 'b') { int n = 0; while (ofdm_host_pipe_buffer(c, n, &p, &cap, &pinned)) n++; *value = n; return OFDM_OK; }
        const char *num = std::strchr(key, ':') + 1;
        char *end = nullptr;
        if (*num < '0' || *num > '9') return OFDM_ERR_INVALID;
        const long i = std::strtol(num, &end, 10);
        if (*end || i > 1000 || !ofdm_host_pipe_buffer(c, (int)i, &p, &cap, &pinned)) return OFDM_ERR_INVALID;
        *value = key[11] == 't' ? (int64_t)(uintptr_t)p : key[10] == 'c' ? (int64_t)cap : pinned;
        return OFDM_OK;
    }
    for (const TuneKey &k : kTuneKeys)
        if (std::strcmp(key, k.name) == 0) { *value = c->tune.*(k.field); return OFDM_OK; }
    return OFDM_ERR_INVALID;
}
int ofdm_last_dispatch(const ofdm_ctx *c, char *buf, size_t n) {
    if (!c || !buf || !n) return OFDM_ERR_INVALID;
    const size_t len = (size_t)c->trace.len < n - 1 ? (size_t)c->trace.len : n - 1;
    std::memcpy(buf, c->trace.buf, len);
    buf[len] = 0;
    return (int)c->trace.len; // the full length, like snprintf
}

int ofdm_dev_alloc(ofdm_ctx *c, size_t bytes, void **dev) {
    if (!c || !dev) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    hipError_t e = hipMalloc(dev, bytes ? bytes : 1);
    if (e != hipSuccess) { c->last_hip = (int)e; *dev = nullptr; return OFDM_ERR_NOMEM; }
    return OFDM_OK;
}
int ofdm_dev_free(ofdm_ctx *c, void *dev) {
    if (!c) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    if (dev) { HIP_TRY(c, hipStreamSynchronize(c->stream)); HIP_TRY(c, hipFree(dev)); }
    return OFDM_OK;
}
int ofdm_memcpy_h2d(ofdm_ctx *c, void *dev, const void *host, size_t bytes) {
    if (!c || (bytes && (!dev || !host))) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    HIP_TRY(c, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    return OFDM_OK;
}
int ofdm_memcpy_d2h(ofdm_ctx *c, void *host, const void *dev, size_t bytes) {
    if (!c || (bytes && (!dev || !host))) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    HIP_TRY(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return OFDM_OK;
}
int ofdm_memset(ofdm_ctx *c, void *dev, int value, size_t bytes) {
    if (!c || (bytes && !dev)) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    HIP_TRY(c, hipMemsetAsync(dev, value, bytes, c->stream));
    return OFDM_OK;
}

int ofdm_symbol_len(const ofdm_ctx *c) { return c ? c->S() : OFDM_ERR_INVALID; }
int ofdm_data_carriers(const ofdm_ctx *c) { return c ? c->carriers() : OFDM_ERR_INVALID; }
int ofdm_bytes_per_symbol(const ofdm_ctx *c) { return c ? c->bytes_per_symbol() : OFDM_ERR_INVALID; }
int64_t ofdm_coded_len(const ofdm_ctx *c, int64_t payload_bytes) {
    if (!c || payload_bytes < 0) return OFDM_ERR_INVALID;
    return coded_len(c->mode, payload_bytes);
}
int64_t ofdm_data_symbols(const ofdm_ctx *c, int64_t payload_bytes) {
    if (!c || payload_bytes < 0) return OFDM_ERR_INVALID;
    int64_t nsym = ((16 + ofdm_coded_len(c, payload_bytes)) * 8 + c->prm.modulation - 1) / c->prm.modulation;
    return (nsym + c->carriers() - 1) / c->carriers();
}
int64_t ofdm_frame_samples(const ofdm_ctx *c, int64_t payload_bytes) {
    if (!c || payload_bytes < 0) return OFDM_ERR_INVALID;
    return (10 + ofdm_data_symbols(c, payload_bytes)) * (int64_t)c->S();
}

// ------------------------------------------------------------------ stage level
int ofdm_fft_batch(ofdm_ctx *c, const ofdm_fc32 *in, ofdm_fc32 *out, int64_t n_vec, int inverse) {
    if (!c || n_vec < 0 || (n_vec && (!in || !out))) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    SymParams p = base_params(c);
    const int N = c->prm.n_fft;
    p.in = reinterpret_cast<const float2 *>(in); p.out = reinterpret_cast<float2 *>(out);
    p.n_frames = n_vec; p.frame_stride = N; p.frame_len = N; p.syms_per_frame = 1; p.in_sym_stride = N; p.in_skip = 0;
    HIP_TRY(c, run_fft(N, p, inverse != 0, c->stream, c->num_cu));
    return OFDM_OK;
}
int ofdm_ifft_cp_batch(ofdm_ctx *c, const ofdm_fc32 *freq, ofdm_fc32 *out, int64_t n_sym) {
    if (!c || n_sym < 0 || (n_sym && (!freq || !out))) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    SymParams p = base_params(c);
    const int N = c->prm.n_fft;
    p.in = reinterpret_cast<const float2 *>(freq); p.out = reinterpret_cast<float2 *>(out);
    p.n_frames = n_sym; p.frame_stride = N; p.frame_len = N; p.syms_per_frame = 1; p.in_sym_stride = N; p.in_skip = 0;
    HIP_TRY(c, run_ifft_cp(N, p, c->stream, c->num_cu));
    return OFDM_OK;
}
int ofdm_tx_symbols_batch(ofdm_ctx *c, const uint8_t *bytes, int64_t n_bytes, ofdm_fc32 *out, int64_t n_sym) {
    if (!c || n_bytes < 0 || n_sym < 0 || (n_sym && !out) || (n_bytes && !bytes)) return OFDM_ERR_INVALID;
    const int bps_bytes = c->bytes_per_symbol();
    if (n_sym * (int64_t)bps_bytes < n_bytes) return OFDM_ERR_INVALID; // every byte must land in a symbol
    if (!n_sym) return OFDM_OK;
    EntryScope scope(c);
    SymParams p = base_params(c);
    p.n_frames = n_sym; p.syms_per_frame = 1;
    p.payload = bytes; p.payload_stride = bps_bytes; p.payload_len = nullptr; p.payload_bytes = bps_bytes;
    p.tx_raw_total = n_bytes;
    p.out = reinterpret_cast<float2 *>(out); p.out_stride_s = c->S(); p.frame_max = nullptr;
    // 64 x 64 two-stage kernel (kernels_n4096.hip; the A/B switch is shared with the RX side)
    if (c->prm.n_fft == 4096) FAST_PATH(c, c->tune.no_demod4096, run_tx4096(p, c->stream, c->num_cu));
    // R x 64 two-stage kernels (kernels_mid.hip; N = 64 is the one-row case)
    if (c->prm.n_fft < 4096) FAST_PATH(c, c->tune.no_mid_kernels, run_tx_mid(c->prm.n_fft, p, c->stream, c->num_cu));
    HIP_TRY(c, run_tx_symbols(c->prm.n_fft, p, c->stream, c->num_cu));
    return OFDM_OK;
}
int ofdm_unprefix_batch(ofdm_ctx *c, const ofdm_fc32 *in, ofdm_fc32 *out, int64_t n_sym) {
    if (!c || n_sym < 0 || (n_sym && (!in || !out))) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    SymParams p = base_params(c);
    const int N = c->prm.n_fft, S = c->S();
    p.in = reinterpret_cast<const float2 *>(in); p.out = reinterpret_cast<float2 *>(out);
    p.n_frames = n_sym; p.frame_stride = S; p.frame_len = S; p.syms_per_frame = 1; p.in_sym_stride = S; p.in_skip = c->prm.cp_len;
    HIP_TRY(c, run_fft(N, p, false, c->stream, c->num_cu));
    return OFDM_OK;
}
int ofdm_qam_map_batch(ofdm_ctx *c, const uint8_t *bytes, int64_t n_bytes, ofdm_fc32 *out) {
    if (!c || n_bytes < 0 || (n_bytes && (!bytes || !out))) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    HIP_TRY(c, run_qam_map(bytes, n_bytes, c->prm.modulation, reinterpret_cast<float2 *>(out), c->stream));
    return OFDM_OK;
}
int ofdm_qam_demap_batch(ofdm_ctx *c, const ofdm_fc32 *sym, int64_t n_sym, uint8_t *bytes, uint8_t *idx) {
    if (!c || n_sym < 0 || (n_sym && !sym)) return OFDM_ERR_INVALID;
    if (n_sym % 8 != 0) return OFDM_ERR_INVALID; // assert_eq!(remainder.len(), 0), src/receiver.rs:153
    EntryScope scope(c);
    HIP_TRY(c, run_qam_demap(reinterpret_cast<const float2 *>(sym), n_sym, c->prm.modulation, bytes, idx, c->stream));
    return OFDM_OK;
}
int ofdm_encode_block_batch(ofdm_ctx *c, const ofdm_fc32 *data, ofdm_fc32 *bins, int64_t n_sym) {
    if (!c || n_sym < 0 || (n_sym && (!data || !bins))) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    HIP_TRY(c, run_encode_block(reinterpret_cast<const float2 *>(data), reinterpret_cast<float2 *>(bins), n_sym,
                                c->prm.n_fft, c->prm.guard_bands, c->stream));
    return OFDM_OK;
}
int ofdm_normalize_batch(ofdm_ctx *c, ofdm_fc32 *x, int64_t n_frames, int64_t frame_stride, int64_t frame_len) {
    if (!c || n_frames < 0 || frame_len < 0 || frame_stride < frame_len || (n_frames && !x)) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    if (!n_frames) return OFDM_OK;
    void *mx;
    int rc = ws_get(c, kWsFrameMax, sizeof(unsigned) * (size_t)n_frames, &mx);
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(mx, 0, sizeof(unsigned) * (size_t)n_frames, c->stream));
    HIP_TRY(c, run_frame_max(reinterpret_cast<float2 *>(x), n_frames, frame_stride, frame_len, (unsigned *)mx, c->stream));
    HIP_TRY(c, run_frame_scale(reinterpret_cast<float2 *>(x), n_frames, frame_stride, frame_len, (unsigned *)mx, c->stream));
    return OFDM_OK;
}
int ofdm_hamming74_encode(ofdm_ctx *c, const uint8_t *in, int64_t n_bytes, uint8_t *out) {
    if (!c || n_bytes < 0 || (n_bytes && (!in || !out))) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    HIP_TRY(c, run_ham_encode(in, 1, 0, nullptr, n_bytes, out, 0, nullptr, c->stream));
    return OFDM_OK;
}
int ofdm_hamming74_decode(ofdm_ctx *c, const uint8_t *in, int64_t n_bytes, uint8_t *out, uint32_t *corrected) {
    if (!c || n_bytes < 0 || (n_bytes >= 7 && (!in || !out))) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    HIP_TRY(c, run_ham_decode(in, n_bytes, out, corrected, c->stream));
    return OFDM_OK;
}
int ofdm_hamming74_decode_soft(ofdm_ctx *c, const int8_t *llr, int64_t n_bits, uint8_t *out) {
    if (!c || n_bits < 0 || (n_bits >= 56 && (!llr || !out))) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    c->trace.add("k_ham_decode_soft");
    HIP_TRY(c, run_ham_decode_soft(llr, n_bits, out, c->stream));
    return OFDM_OK;
}

// The survivor slabs of a Viterbi launch over n_frames frames of at most max_steps steps: the grid, and p's slab size and workspace
static int viterbi_survivors(ofdm_ctx *c, int64_t n_frames, int64_t max_steps, ViterbiParams &p, long long *blocks) {
    viterbi_k7_plan(n_frames, max_steps, c->num_cu, &c->tune, blocks, &p.slab_words);
    void *w_surv = nullptr;
    const int rc = ws_get(c, kWsSurvivors, (size_t)(*blocks * 4 * p.slab_words) * sizeof(unsigned long long), &w_surv);
    p.surv = (unsigned long long *)w_surv;
    return rc;
}
// int32 path metrics, not renormalised: 2^20 steps of at most 256 each stay clear of the floor of the excluded states (-2^30)
static const int64_t kViterbiMaxSteps = 1ll << 20;
int ofdm_conv_k7_encode(ofdm_ctx *c, const uint8_t *in, int64_t n_frames, int64_t in_stride, int64_t n_bytes, uint8_t *out,
                        int64_t out_stride) {
    if (!c || n_frames < 0 || n_bytes < 0 || in_stride < n_bytes || out_stride < 2 * (n_bytes + 1)) return OFDM_ERR_INVALID;
    if (n_frames && (!out || (n_bytes && !in))) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    c->trace.add("k_conv_encode");
    HIP_TRY(c, run_conv_encode(in, n_frames, in_stride, nullptr, n_bytes, out, out_stride, nullptr, c->stream));
    return OFDM_OK;
}
int ofdm_conv_k7_decode_soft(ofdm_ctx *c, const int8_t *llr, int64_t n_frames, int64_t llr_stride, int64_t n_steps, int32_t terminated,
                             uint8_t *out, int64_t out_stride) {
    if (!c || n_frames < 0 || n_steps < 0 || llr_stride < 2 * n_steps || out_stride < n_steps / 8) return OFDM_ERR_INVALID;
    if (n_steps > kViterbiMaxSteps) return OFDM_ERR_UNSUPPORTED;
    if (n_frames && n_steps && (!llr || (n_steps >= 8 && !out))) return OFDM_ERR_INVALID;
    if (!n_frames || !n_steps) return OFDM_OK;
    EntryScope scope(c);
    ViterbiParams p;
    long long blocks;
    int rc = viterbi_survivors(c, n_frames, n_steps, p, &blocks);
    if (rc) return rc;
    p.llr = llr; p.llr_stride = llr_stride; p.n_frames = n_frames; p.out = out; p.out_stride = out_stride;
    p.n_steps = (int)n_steps; p.terminated = terminated != 0;
    c->trace.add("k_viterbi_k7");
    HIP_TRY(c, run_viterbi_k7(p, blocks, c->stream));
    return OFDM_OK;
}

int64_t ofdm_conv_k7_kept_bits(int64_t n_steps, int32_t rate) {
    if (n_steps < 0 || rate < 0 || rate >= kConvRates) return OFDM_ERR_INVALID;
    return conv_kept_bits(n_steps, rate);
}
int ofdm_conv_k7_encode_punctured(ofdm_ctx *c, const uint8_t *in, int64_t n_frames, int64_t in_stride, int64_t n_bytes, int32_t rate,
                                  uint8_t *out, int64_t out_stride) {
    if (!c || n_frames < 0 || n_bytes < 0 || rate < 0 || rate >= kConvRates) return OFDM_ERR_INVALID;
    if (in_stride < n_bytes || out_stride < conv_body_len(n_bytes, rate)) return OFDM_ERR_INVALID;
    if (n_frames && (!out || (n_bytes && !in))) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    c->trace.add("k_conv_encode_p");
    HIP_TRY(c, run_conv_encode_p(in, n_frames, in_stride, nullptr, n_bytes, rate, 0, out, out_stride, nullptr, c->stream));
    return OFDM_OK;
}
int ofdm_conv_k7_decode_punctured(ofdm_ctx *c, const int8_t *llr, int64_t n_frames, int64_t llr_stride, int64_t n_steps, int32_t rate,
                                  int32_t terminated, uint8_t *out, int64_t out_stride) {
    if (!c || n_frames < 0 || n_steps < 0 || rate < 0 || rate >= kConvRates) return OFDM_ERR_INVALID;
    if (n_steps > kViterbiMaxSteps) return OFDM_ERR_UNSUPPORTED;
    if (llr_stride < conv_kept_bits(n_steps, rate) || out_stride < n_steps / 8) return OFDM_ERR_INVALID;
    if (n_frames && n_steps && (!llr || (n_steps >= 8 && !out))) return OFDM_ERR_INVALID;
    if (!n_frames || !n_steps) return OFDM_OK;
    EntryScope scope(c);
    ViterbiFParams p;
    long long blocks;
    int rc = viterbi_survivors(c, n_frames, n_steps, p, &blocks);
    if (rc) return rc;
    p.llr = llr; p.llr_stride = llr_stride; p.n_frames = n_frames; p.out = out; p.out_stride = out_stride;
    p.n_steps = (int)n_steps; p.terminated = terminated != 0; p.rate = rate;
    c->trace.add("k_viterbi_k7f");
    HIP_TRY(c, run_viterbi_k7f(p, blocks, c->stream));
    return OFDM_OK;
}

// ---- the outer layers of a mode (ModePlan::outer; the length maps are outer_coded_bytes / outer_row_limit in ofdm_ctx.hpp).  One kernel
// each way: on transmit rows + optional lengths -> longer rows + optional lengths, on receive rows -> the rows of the layer outside.
// The stage entry points below and the chains of the frame modes launch them through the same four functions.
namespace {
struct LayerCall {
    const uint8_t *in; int64_t n_frames, in_stride, n_in; const int32_t *in_len;  // rows of n_in bytes (row f: in_len[f] when given)
    uint8_t *out; int64_t out_stride; int32_t *out_len;
    int32_t *aux, *status_rw; // receive: ok / corrected per row (stage mode), the frames' status (chain mode)
};
hipError_t fcs_wrap(ofdm_ctx *c, const LayerCall &r) {
    FcsWrapParams p;
    p.in = r.in; p.n_frames = r.n_frames; p.in_stride = r.in_stride; p.n_bytes = r.n_in; p.in_len = r.in_len; p.out = r.out; p.out_stride = r.out_stride;
    p.out_len = r.out_len;
    return run_fcs_wrap(p, c->num_cu, &c->tune, c->stream);
}
hipError_t fcs_check(ofdm_ctx *c, const LayerCall &r) {
    FcsCheckParams p;
    p.row = r.in; p.n_frames = r.n_frames; p.row_stride = r.in_stride; p.n_row = r.n_in; p.row_len = r.in_len; p.out = r.out; p.out_stride = r.out_stride;
    p.out_len = r.out_len; p.ok = r.aux; p.status_rw = r.status_rw;
    return run_fcs_check(p, c->num_cu, &c->tune, c->stream);
}
hipError_t rs_encode(ofdm_ctx *c, const LayerCall &r) {
    Rs255EncodeParams p;
    p.in = r.in; p.n_frames = r.n_frames; p.in_stride = r.in_stride; p.n_bytes = r.n_in; p.in_len = r.in_len; p.out = r.out; p.out_stride = r.out_stride;
    p.out_len = r.out_len;
    return run_rs255_encode(p, c->num_cu, &c->tune, c->stream);
}
hipError_t rs_decode(ofdm_ctx *c, const LayerCall &r) {
    Rs255DecodeParams p;
    p.code = r.in; p.n_frames = r.n_frames; p.code_stride = r.in_stride; p.n_code = r.n_in; p.code_len = r.in_len; p.out = r.out; p.out_stride = r.out_stride;
    p.out_len = r.out_len; p.corrected = r.aux; p.status_rw = r.status_rw;
    return run_rs255_decode(p, c->num_cu, &c->tune, c->stream);
}
struct OuterStage {
    WsRole tx_rows, tx_len, rx_rows;
    const char *tx_name, *rx_name;
    hipError_t (*encode)(ofdm_ctx *, const LayerCall &), (*decode)(ofdm_ctx *, const LayerCall &);
    int64_t rx_max_row; // the longest row the receive kernel takes
};
const OuterStage kOuter[] = { // indexed by OuterLayer
    {kWsTxFcsRows, kWsTxFcsLen, kWsRxFcsRows, "k_fcs_wrap", "k_fcs_check", fcs_wrap, fcs_check, 0x7fffffffll}, // its length word is 32 bits
    {kWsTxRsRows, kWsTxRsLen, kWsRxRsRows, "k_rs255_encode", "k_rs255_decode", rs_encode, rs_decode, INT64_MAX},
};
} // namespace

// outer Reed-Solomon(255,223) on device rows (kernels_rs.hip)
int ofdm_rs255_encode_batch(ofdm_ctx *c, const uint8_t *in, int64_t n_frames, int64_t in_stride, const int32_t *in_len, int64_t n_bytes,
                            uint8_t *out, int64_t out_stride) {
    if (!c || n_frames < 0 || n_bytes < 0 || in_stride < n_bytes || out_stride < ofdm_rs255_encoded_len(n_bytes)) return OFDM_ERR_INVALID;
    if (n_frames && (!out || (n_bytes && !in))) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    c->trace.add("k_rs255_encode");
    HIP_TRY(c, rs_encode(c, LayerCall{in, n_frames, in_stride, n_bytes, in_len, out, out_stride, nullptr, nullptr, nullptr}));
    return OFDM_OK;
}
int ofdm_rs255_decode_batch(ofdm_ctx *c, const uint8_t *code, int64_t n_frames, int64_t code_stride, const int32_t *code_len, int64_t n_code,
                            uint8_t *out, int64_t out_stride, int32_t *out_len, int32_t *corrected) {
    if (!c || n_frames < 0 || n_code < 0 || code_stride < n_code || out_stride < ofdm_rs255_decoded_len(n_code)) return OFDM_ERR_INVALID;
    if (n_frames && (!out || (n_code && !code))) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    c->trace.add("k_rs255_decode");
    HIP_TRY(c, rs_decode(c, LayerCall{code, n_frames, code_stride, n_code, code_len, out, out_stride, out_len, corrected, nullptr}));
    return OFDM_OK;
}

// LDPC(648) on device rows (kernels_ldpc.hip): rows of n_cw plain code words of K = ofdm_ldpc648_info_bytes(rate) info bytes, no
// frame rule
int ofdm_ldpc648_encode_rate_batch(ofdm_ctx *c, const uint8_t *in, int64_t n_frames, int64_t in_stride, int64_t n_cw, int32_t rate, uint8_t *out,
                                   int64_t out_stride) {
    if (!c || rate < 0 || rate >= kLdpcRates || n_frames < 0 || n_cw < 0 || n_cw > (int64_t)1 << 40) return OFDM_ERR_INVALID;
    if (in_stride < kLdpcCodes[rate].info_bytes * n_cw || out_stride < kLdpcCodeBytes * n_cw) return OFDM_ERR_INVALID;
    if (n_frames && n_cw && (!in || !out)) return OFDM_ERR_INVALID;
    if (!n_frames || !n_cw) return OFDM_OK;
    EntryScope scope(c);
    LdpcEncodeParams p;
    p.in = in; p.n_frames = n_frames; p.in_stride = in_stride; p.n_cw = n_cw; p.out = out; p.out_stride = out_stride;
    c->trace.add(ldpc_encode_name(rate));
    HIP_TRY(c, run_ldpc_encode(p, rate, c->num_cu, &c->tune, c->stream));
    return OFDM_OK;
}
int ofdm_ldpc648_decode_rate_batch(ofdm_ctx *c, const int8_t *llr, int64_t n_frames, int64_t llr_stride, int64_t n_cw, int32_t max_iter,
                                   int32_t rate, uint8_t *out, int64_t out_stride, int32_t *iters) {
    if (!c || rate < 0 || rate >= kLdpcRates || n_frames < 0 || n_cw < 0 || n_cw > (int64_t)1 << 40 || max_iter < 1 || max_iter > kLdpcMaxIterLimit)
        return OFDM_ERR_INVALID;
    if (llr_stride < kLdpcSentBits * n_cw || out_stride < kLdpcCodes[rate].info_bytes * n_cw) return OFDM_ERR_INVALID;
    if (n_frames && n_cw && (!llr || !out)) return OFDM_ERR_INVALID;
    if (!n_frames || !n_cw) return OFDM_OK;
    EntryScope scope(c);
    LdpcDecodeParams p;
    p.llr = llr; p.n_frames = n_frames; p.llr_stride = llr_stride; p.n_cw = n_cw; p.max_iter = max_iter; p.out = out; p.out_stride = out_stride;
    p.iters = iters;
    c->trace.add(ldpc_decode_name(rate));
    HIP_TRY(c, run_ldpc_decode(p, rate, c->num_cu, &c->tune, c->stream));
    return OFDM_OK;
}

// rate 1/2 by its own names
int ofdm_ldpc648_encode_batch(ofdm_ctx *c, const uint8_t *in, int64_t n_frames, int64_t in_stride, int64_t n_cw, uint8_t *out, int64_t out_stride) {
    return ofdm_ldpc648_encode_rate_batch(c, in, n_frames, in_stride, n_cw, 0, out, out_stride);
}
int ofdm_ldpc648_decode_batch(ofdm_ctx *c, const int8_t *llr, int64_t n_frames, int64_t llr_stride, int64_t n_cw, int32_t max_iter,
                              uint8_t *out, int64_t out_stride, int32_t *iters) {
    return ofdm_ldpc648_decode_rate_batch(c, llr, n_frames, llr_stride, n_cw, max_iter, 0, out, out_stride, iters);
}

// CRC-32 frame check on device rows (kernels_fcs.hip)
int ofdm_fcs_wrap_batch(ofdm_ctx *c, const uint8_t *in, int64_t n_frames, int64_t in_stride, const int32_t *in_len, int64_t n_bytes,
                        uint8_t *out, int64_t out_stride, int32_t *out_len) {
    if (!c || n_frames < 0 || n_bytes < 0 || in_stride < n_bytes || out_stride - OFDM_FCS_OVERHEAD < n_bytes) return OFDM_ERR_INVALID;
    if (n_bytes > 0x7fffffffll - OFDM_FCS_OVERHEAD) return OFDM_ERR_UNSUPPORTED; // the length word and out_len are 32 bits
    if (n_frames && (!out || (n_bytes && !in))) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    c->trace.add("k_fcs_wrap");
    HIP_TRY(c, fcs_wrap(c, LayerCall{in, n_frames, in_stride, n_bytes, in_len, out, out_stride, out_len, nullptr, nullptr}));
    return OFDM_OK;
}
int ofdm_fcs_check_batch(ofdm_ctx *c, const uint8_t *row, int64_t n_frames, int64_t row_stride, const int32_t *row_len, int64_t n_row,
                         uint8_t *out, int64_t out_stride, int32_t *out_len, int32_t *ok) {
    if (!c || n_frames < 0 || n_row < 0 || row_stride < n_row || out_stride < 0 || out_stride < n_row - OFDM_FCS_OVERHEAD) return OFDM_ERR_INVALID;
    if (n_row > 0x7fffffffll) return OFDM_ERR_UNSUPPORTED;
    if (n_frames && ((n_row > OFDM_FCS_OVERHEAD && !out) || (n_row && !row))) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    c->trace.add("k_fcs_check");
    HIP_TRY(c, fcs_check(c, LayerCall{row, n_frames, row_stride, n_row, row_len, out, out_stride, out_len, ok, nullptr}));
    return OFDM_OK;
}

// Schmidl-Cox parameters of a batch; false when no lag fits the capture (nothing can synchronise)
static bool sc_make_params(ofdm_ctx *c, const float2 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                           int64_t n_lags, int32_t *d_hat, double *f_delta, float *metric, ScParams &p) {
    const int L = c->S(), W = c->prm.sync_window_reps * L;
    const int64_t valid = frame_len - W - L + 1;
    if (valid <= 0) return false;
    if (n_lags <= 0 || n_lags > valid) n_lags = valid;
    p.in = in; p.n_frames = n_frames; p.frame_stride = frame_stride; p.frame_len = frame_len; p.n_lags = n_lags;
    p.L = L; p.W = W; p.threshold = c->sync_threshold_f64 > 0.0 ? c->sync_threshold_f64 : (double)c->prm.sync_threshold;
    p.d_hat = d_hat; p.f_delta = f_delta; p.metric = metric;
    p.tiles_per_frame = 1; p.mode = 0;
    p.tune = &c->tune; p.trace = &c->trace;
    c->sc_stats = ScStats();
    c->sc_stats.dev = c->d_stats;
    p.stats = &c->sc_stats;
    return true;
}

static int sc_run_impl(ofdm_ctx *c, const float2 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                       int64_t n_lags, int32_t *d_hat, double *f_delta, float *metric, bool tail_mapped) {
    ScParams p;
    p.tail_mapped = tail_mapped;
    if (!sc_make_params(c, in, n_frames, frame_stride, frame_len, n_lags, d_hat, f_delta, metric, p)) { // no lag fits
        HIP_TRY(c, hipMemsetAsync(d_hat, 0xFF, sizeof(int32_t) * (size_t)n_frames, c->stream));
        if (f_delta) HIP_TRY(c, hipMemsetAsync(f_delta, 0, sizeof(double) * (size_t)n_frames, c->stream));
        if (metric) HIP_TRY(c, hipMemsetAsync(metric, 0, sizeof(float) * (size_t)n_frames, c->stream));
        return OFDM_OK;
    }
    n_lags = p.n_lags;
    // N = 64 (L = 80): k_sc80, every lag exactly in one streaming pass, whatever the slot length; its A/B predecessor (and the path
    // of unaligned batches): one-tile frames through the coarse-then-fine f32 filter + exact f64 decisions (k_sc_cf)
    if (sc_fast_ok(p) || (!c->tune.no_sc80 && sc80_wanted(p))) {
        void *wsp;
        int rc = ws_get(c, kWsSearch, sc_fast_workspace_bytes(n_frames, p.n_lags), &wsp);
        if (rc) return rc;
        HIP_TRY(c, run_sc_fast(p, wsp, c->num_cu, c->stream));
        return OFDM_OK;
    }
    // L = 160 .. 1280 (N = 128 .. 1024): ONE streaming pass per frame -- exact sums at every 10th lag from running prefixes, lag-by-lag
    // evaluation only where a bound allows a crossing / a new maximum -- that stops once the peak window is closed (kernels_scstream.hip)
    if (sc_stream_ok(p) && !c->tune.no_sc_stream) {
        HIP_TRY(c, run_sc_stream(p, c->num_cu, c->stream));
        return OFDM_OK;
    }
    // long periods (N >= 128): one streaming pass for chunk sums, then an exact search only where the chunk bounds allow a
    // crossing / a new maximum (kernels_scbig.hip); LDS footprint independent of L, so N = 4096 works too
    const bool one_small_tile = n_lags <= sc_tile_lags() && sc_lds_bytes(p) <= 64 * 1024; // bounded search, window in LDS: k_sc_tile reads less
    if (sc_big_ok(p) && !one_small_tile && !c->tune.no_sc_big) {
        void *wsp;
        int rc = ws_get(c, kWsSearch, sc_big_workspace_bytes(p), &wsp);
        if (rc) return rc;
        HIP_TRY(c, run_sc_big(p, wsp, c->num_cu, c->stream));
        return OFDM_OK;
    }
    if (sc_lds_bytes(p) > 160 * 1024) return OFDM_ERR_UNSUPPORTED; // window does not fit one CU's LDS
    const int CH = sc_tile_lags();
    const int64_t tiles = (n_lags + CH - 1) / CH;
    if (tiles > 0x7fffffff) return OFDM_ERR_INVALID;
    if (tiles == 1) {
        HIP_TRY(c, run_sc(p, c->stream));
        return OFDM_OK;
    }
    // long captures: first threshold crossing per tile -> per frame -> peak search from there (one tile)
    void *cross, *d1;
    int rc = ws_get(c, kWsSearch, sizeof(long long) * (size_t)(n_frames * tiles), &cross);
    if (rc) return rc;
    rc = ws_get(c, kWsSearchD1, sizeof(int32_t) * (size_t)n_frames, &d1);
    if (rc) return rc;
    p.tiles_per_frame = (int)tiles; p.mode = 1; p.cross = (long long *)cross;
    HIP_TRY(c, run_sc(p, c->stream));
    HIP_TRY(c, run_sc_min_cross((const long long *)cross, (int)tiles, n_frames, (int32_t *)d1, c->stream));
    p.tiles_per_frame = 1; p.mode = 2; p.lag_base = (const int32_t *)d1;
    HIP_TRY(c, run_sc(p, c->stream));
    return OFDM_OK;
}

int ofdm_abi_sc_run(ofdm_ctx *c, const float2 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                    int64_t n_lags, int32_t *d_hat, double *f_delta, float *metric) {
    // Tight rows of odd length (stride == length): k_sc80 is given an even slot length, i.e. reads one sample past an odd slot -- the next
    // row's first one, except behind the last row.  That row goes through the general paths on its own, the others through k_sc80.
    if (n_frames > 1 && (frame_len & 1) && frame_stride == frame_len && !c->tune.no_sc80) {
        ScParams head;
        head.tail_mapped = true;
        if (sc_make_params(c, in, n_frames - 1, frame_stride, frame_len, n_lags, d_hat, f_delta, metric, head) && sc80_wanted(head)) {
            int rc = sc_run_impl(c, in, n_frames - 1, frame_stride, frame_len, n_lags, d_hat, f_delta, metric, true);
            if (rc) return rc;
            const int64_t l = n_frames - 1;
            return sc_run_impl(c, in + l * frame_stride, 1, frame_len, frame_len, n_lags, d_hat + l, f_delta ? f_delta + l : nullptr,
                               metric ? metric + l : nullptr, false);
        }
    }
    return sc_run_impl(c, in, n_frames, frame_stride, frame_len, n_lags, d_hat, f_delta, metric, false);
}

int ofdm_sc_correlate_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_frames, int64_t frame_stride,
                            int64_t frame_len, int64_t n_lags, int32_t *d_hat, double *f_delta, float *metric) {
    if (!c || n_frames < 0 || frame_len <= 0 || frame_stride < 0 || (n_frames && (!in || !d_hat))) return OFDM_ERR_INVALID;
    if (n_frames > 1 && frame_stride <= 0) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    return ofdm_abi_sc_run(c, reinterpret_cast<const float2 *>(in), n_frames, frame_stride, frame_len, n_lags, d_hat, f_delta, metric);
}
int ofdm_xcorr_batch(ofdm_ctx *c, const ofdm_fc32 *a, int64_t n_frames, int64_t a_stride, int64_t a_len, const ofdm_fc32 *b,
                     int32_t nb, int32_t *idx_max, float *peak, ofdm_fc32 *out, int64_t out_stride) {
    if (!c || n_frames < 0 || a_len <= 0 || nb <= 0 || nb > 8192 || nb > a_len || a_len > 0x3fffffff) return OFDM_ERR_INVALID;
    if (n_frames && (!a || !b || !idx_max)) return OFDM_ERR_INVALID;
    if (n_frames > 1 && a_stride <= 0) return OFDM_ERR_INVALID;
    if (out && out_stride < 2 * a_len - 1) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    void *w;
    int rc = ws_get(c, kWsSearch, xcorr_workspace_bytes(n_frames, a_len, nb), &w);
    if (rc) return rc;
    HIP_TRY(c, run_xcorr(reinterpret_cast<const float2 *>(a), n_frames, a_stride, a_len, reinterpret_cast<const float2 *>(b), nb, w,
                         idx_max, peak, reinterpret_cast<float2 *>(out), out_stride, c->num_cu, c->stream));
    return OFDM_OK;
}

int ofdm_frequency_correction_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_pairs, int64_t stride,
                                    int64_t right_offset, double *f_delta) {
    if (!c || n_pairs < 0 || (n_pairs && (!in || !f_delta))) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    HIP_TRY(c, run_freq_correction(reinterpret_cast<const float2 *>(in), n_pairs, stride, right_offset, c->S(), f_delta, c->stream));
    return OFDM_OK;
}
int ofdm_cfo_rotate_batch(ofdm_ctx *c, ofdm_fc32 *x, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                          const double *f_delta, const int32_t *first_index) {
    if (!c || n_frames < 0 || frame_len < 0 || (n_frames && (!x || !f_delta))) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    HIP_TRY(c, run_cfo_rotate(reinterpret_cast<float2 *>(x), n_frames, frame_stride, frame_len, f_delta, first_index, c->stream));
    return OFDM_OK;
}
int ofdm_estimate_channel_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_frames, int64_t frame_stride,
                                int64_t frame_len, const int32_t *offset, const double *f_delta, ofdm_fc32 *hk) {
    if (!c || n_frames < 0 || frame_len <= 0 || (n_frames && (!in || !hk))) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    SymParams p = rx_params(c, reinterpret_cast<const float2 *>(in), n_frames, frame_stride, frame_len, offset, f_delta);
    p.out = reinterpret_cast<float2 *>(hk);
    HIP_TRY(c, run_chest(c->prm.n_fft, p, c->stream, c->num_cu));
    if (c->prm.chest_mode == OFDM_CHEST_WLS && n_frames) return chest_smooth_run(c, p.out, n_frames, p.out);
    return OFDM_OK;
}

int ofdm_chest_matrix(int32_t n_fft, int32_t cp_len, const double *training, double *rinv) {
    if (!valid_nfft(n_fft) || cp_len != n_fft / 4 || !rinv) return OFDM_ERR_INVALID;
    std::vector<double> trn(2 * (size_t)n_fft);
    if (training) std::memcpy(trn.data(), training, sizeof(double) * trn.size());
    else ofdm_default_pilots(n_fft, cp_len, nullptr, trn.data());
    std::vector<cd> B;
    if (!chest_rinv(n_fft, trn.data(), B)) return OFDM_ERR_INVALID;
    for (size_t i = 0; i < B.size(); i++) { rinv[2 * i] = B[i].re; rinv[2 * i + 1] = B[i].im; }
    return OFDM_OK;
}
int ofdm_chest_window(const ofdm_ctx *c, int32_t *first_tap, int32_t *n_taps) {
    if (!c || !first_tap || !n_taps) return OFDM_ERR_INVALID;
    *first_tap = -(c->prm.cp_len / 4);
    *n_taps = c->prm.cp_len;
    return OFDM_OK;
}
int ofdm_chest_smooth_batch(ofdm_ctx *c, const ofdm_fc32 *hk_in, int64_t n_frames, ofdm_fc32 *hk_out) {
    if (!c || n_frames < 0 || (n_frames && (!hk_in || !hk_out))) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    return chest_smooth_run(c, reinterpret_cast<const float2 *>(hk_in), n_frames, reinterpret_cast<float2 *>(hk_out));
}

static int demod_run(ofdm_ctx *c, const float2 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                     int first_symbol, int syms_per_frame, const int32_t *offset, const double *f_delta,
                     const int32_t *nsym_frame, const float2 *hk, int64_t hk_stride, uint8_t *out, int64_t out_stride,
                     float2 *soft) {
    SymParams p = rx_params(c, in, n_frames, frame_stride, frame_len, offset, f_delta, nsym_frame, out, out_stride);
    p.first_symbol = first_symbol; p.syms_per_frame = syms_per_frame; p.in_sym_stride = c->S(); p.in_skip = c->prm.cp_len;
    p.hk = hk; p.hk_stride = hk_stride; p.soft = soft;
    const int N = c->prm.n_fft;
    // regular, aligned streams take the wave-centric fast path (kernels_n64.hip)
    if (N == 64) FAST_PATH(c, c->tune.no_fast64, run_demod64_fast(p, c->stream, c->num_cu));
    // 64 x 64 two-stage kernel for regular streams (kernels_n4096.hip)
    if (N == 4096) FAST_PATH(c, c->tune.no_demod4096, run_demod4096(p, c->stream, c->num_cu));
    // R x 64 two-stage kernels for regular streams (kernels_mid.hip)
    if (N > 64 && N < 4096) FAST_PATH(c, c->tune.no_mid_kernels, run_demod_mid(N, p, c->stream, c->num_cu));
    HIP_TRY(c, run_demod(c->prm.n_fft, p, c->stream, c->num_cu));
    return OFDM_OK;
}

int ofdm_rx_demod_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                        int32_t first_symbol, int32_t syms_per_frame, const int32_t *offset, const double *f_delta,
                        const ofdm_fc32 *hk, int64_t hk_stride, uint8_t *out, int64_t out_stride, ofdm_fc32 *soft) {
    if (!c || n_frames < 0 || syms_per_frame < 0 || first_symbol < 0 || frame_len <= 0) return OFDM_ERR_INVALID;
    if (n_frames && syms_per_frame && (!in || !out)) return OFDM_ERR_INVALID;
    if (out_stride < (int64_t)syms_per_frame * c->bytes_per_symbol()) return OFDM_ERR_INVALID;
    if (hk && hk_stride != 0 && hk_stride != c->prm.n_fft) return OFDM_ERR_INVALID;
    if (!n_frames || !syms_per_frame) return OFDM_OK;
    EntryScope scope(c);
    return demod_run(c, reinterpret_cast<const float2 *>(in), n_frames, frame_stride, frame_len, first_symbol,
                     syms_per_frame, offset, f_delta, nullptr, reinterpret_cast<const float2 *>(hk), hk_stride, out,
                     out_stride, reinterpret_cast<float2 *>(soft));
}

// int8 max-log LLRs in place of the hard bytes of ofdm_rx_demod_batch: k_sym<llr> (no shape-specialised kernel has the epilogue yet)
static int llr_run(ofdm_ctx *c, const float2 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len, int first_symbol,
                   int syms_per_frame, const int32_t *offset, const double *f_delta, const int32_t *nsym_frame, const float2 *hk,
                   int64_t hk_stride, float llr_scale, int8_t *llr, int64_t llr_stride, uint8_t *hard, int64_t hard_stride,
                   const float *bin_weight = nullptr, int64_t bin_weight_stride = 0) {
    SymParams p = rx_params(c, in, n_frames, frame_stride, frame_len, offset, f_delta, nsym_frame, hard, hard_stride);
    p.first_symbol = first_symbol; p.syms_per_frame = syms_per_frame; p.in_sym_stride = c->S(); p.in_skip = c->prm.cp_len;
    p.hk = hk; p.hk_stride = hk_stride;
    p.llr = llr; p.llr_scale = llr_scale; p.llr_stride = llr_stride;
    if (bin_weight) { // EXT-11: k_sym<llrw>
        p.bin_weight = bin_weight; p.bin_weight_stride = bin_weight_stride;
        HIP_TRY(c, run_llrw(c->prm.n_fft, p, c->stream, c->num_cu));
        return OFDM_OK;
    }
    HIP_TRY(c, run_llr(c->prm.n_fft, p, c->stream, c->num_cu));
    return OFDM_OK;
}
int ofdm_rx_llr_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                      int32_t first_symbol, int32_t syms_per_frame, const int32_t *offset, const double *f_delta,
                      const ofdm_fc32 *hk, int64_t hk_stride, float llr_scale, int8_t *llr, int64_t llr_stride) {
    return ofdm_rx_llr_weighted_batch(c, in, n_frames, frame_stride, frame_len, first_symbol, syms_per_frame, offset, f_delta, hk, hk_stride,
                                      llr_scale, llr, llr_stride, nullptr, 0);
}
// EXT-11: the same with per-bin weights (k_sym<llrw>); without them it is ofdm_rx_llr_batch
int ofdm_rx_llr_weighted_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                               int32_t first_symbol, int32_t syms_per_frame, const int32_t *offset, const double *f_delta,
                               const ofdm_fc32 *hk, int64_t hk_stride, float llr_scale, int8_t *llr, int64_t llr_stride,
                               const float *bin_weight, int64_t bin_weight_stride) {
    if (!c || n_frames < 0 || syms_per_frame < 0 || first_symbol < 0 || frame_len <= 0) return OFDM_ERR_INVALID;
    if (!(llr_scale > 0.f && llr_scale <= 3.402823466e38f)) return OFDM_ERR_INVALID; // finite and > 0 (NaN fails both)
    if (n_frames && syms_per_frame && (!in || !llr)) return OFDM_ERR_INVALID;
    if (llr_stride < (int64_t)syms_per_frame * c->carriers() * c->prm.modulation) return OFDM_ERR_INVALID;
    if (hk && hk_stride != 0 && hk_stride != c->prm.n_fft) return OFDM_ERR_INVALID;
    if (bin_weight && bin_weight_stride != 0 && bin_weight_stride != c->prm.n_fft) return OFDM_ERR_INVALID;
    if (!n_frames || !syms_per_frame) return OFDM_OK;
    EntryScope scope(c);
    return llr_run(c, reinterpret_cast<const float2 *>(in), n_frames, frame_stride, frame_len, first_symbol, syms_per_frame, offset,
                   f_delta, nullptr, reinterpret_cast<const float2 *>(hk), hk_stride, llr_scale, llr, llr_stride, nullptr, 0,
                   bin_weight, bin_weight_stride);
}

// EXT-11 noise-aware LLR weights: one launch of k_noise_bins, a row of n_fft floats per frame (include/ofdm_hip.h,
// tests/noise_weight_ref.py)
static int noise_bins_run(ofdm_ctx *c, const float2 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len, const int32_t *offset,
                          const double *f_delta, const int32_t *status, float *nvar, float *weight) {
    NoiseBinsParams p;
    p.tune = &c->tune; p.trace = &c->trace;
    p.in = in; p.n_frames = n_frames; p.frame_stride = frame_stride; p.frame_len = frame_len;
    p.sym_len = c->S();
    p.offset = offset; p.f_delta = f_delta; p.status = status;
    p.tw = c->d_tw;
    p.nvar = nvar; p.weight = weight;
    HIP_TRY(c, run_noise_bins(c->prm.n_fft, p, c->stream, c->num_cu));
    return OFDM_OK;
}
int ofdm_rx_noise_bins_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len, const int32_t *offset,
                             const double *f_delta, const int32_t *status, float *nvar, float *weight) {
    if (!c || n_frames < 0 || frame_len <= 0 || frame_stride < 0) return OFDM_ERR_INVALID;
    if (n_frames && (!in || !offset)) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    return noise_bins_run(c, reinterpret_cast<const float2 *>(in), n_frames, frame_stride, frame_len, offset, f_delta, status, nvar, weight);
}
int ofdm_set_llr_weight(ofdm_ctx *c, int32_t mode) {
    if (!c || (mode != OFDM_LLRW_CHANNEL && mode != OFDM_LLRW_NOISE)) return OFDM_ERR_INVALID;
    c->llr_weight = mode;
    return OFDM_OK;
}
int ofdm_get_llr_weight(const ofdm_ctx *c, int32_t *mode) {
    if (!c || !mode) return OFDM_ERR_INVALID;
    *mode = c->llr_weight;
    return OFDM_OK;
}
// The weights of the decode chains under OFDM_LLRW_NOISE: k_noise_bins over the chain's rows (offset, f_delta and status as the front
// end left them), behind the channel estimate, into the context's workspace; *q stays nullptr under OFDM_LLRW_CHANNEL
static int rx_noise_weights(ofdm_ctx *c, const float2 *in, int64_t n_rows, int64_t frame_stride, int64_t frame_len, const int32_t *offset,
                            const double *f_delta, const int32_t *status, const float **q) {
    *q = nullptr;
    if (c->llr_weight != OFDM_LLRW_NOISE) return OFDM_OK;
    void *w_q;
    int rc;
    if ((rc = ws_get(c, kWsNoiseWeight, sizeof(float) * (size_t)c->prm.n_fft * (size_t)n_rows, &w_q))) return rc;
    if ((rc = noise_bins_run(c, in, n_rows, frame_stride, frame_len, offset, f_delta, status, nullptr, (float *)w_q))) return rc;
    *q = (const float *)w_q;
    return OFDM_OK;
}

// EXT-6 link quality: one launch of k_linkq, a row per frame (include/ofdm_hip.h, tests/quality_ref.py)
static int linkq_run(ofdm_ctx *c, const float2 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len, int32_t first_symbol,
                     int32_t syms_per_frame, const int32_t *n_points, const int32_t *offset, const double *f_delta, const float2 *hk,
                     int64_t hk_stride, const int32_t *status, float *quality) {
    LinkqParams p;
    p.tune = &c->tune; p.trace = &c->trace;
    p.in = in; p.n_frames = n_frames; p.frame_stride = frame_stride; p.frame_len = frame_len;
    p.first_symbol = first_symbol; p.syms_per_frame = syms_per_frame; p.sym_len = c->S();
    p.n_points = n_points; p.offset = offset; p.f_delta = f_delta; p.status = status;
    p.hk = hk; p.hk_stride = hk_stride; p.tw = c->d_tw;
    p.bps = c->prm.modulation; p.guard = c->prm.guard_bands;
    const int N = c->prm.n_fft;
    p.inv_t2 = linkq_inv_t2(c->training.data(), N, p.guard);
    p.es = linkq_es(p.bps);
    p.quality = quality;
    HIP_TRY(c, run_linkq(N, p, c->stream, c->num_cu));
    return OFDM_OK;
}
int ofdm_rx_quality_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                          int32_t first_symbol, int32_t syms_per_frame, const int32_t *n_points, const int32_t *offset,
                          const double *f_delta, const ofdm_fc32 *hk, int64_t hk_stride, const int32_t *status, float *quality) {
    if (!c || n_frames < 0 || syms_per_frame < 0 || first_symbol < 0 || frame_len <= 0 || frame_stride < 0) return OFDM_ERR_INVALID;
    if (n_frames && (!in || !quality)) return OFDM_ERR_INVALID;
    if (hk && hk_stride != 0 && hk_stride != c->prm.n_fft) return OFDM_ERR_INVALID;
    if ((int64_t)syms_per_frame * c->carriers() > (1ll << 24)) return OFDM_ERR_INVALID; // OFDM_Q_POINTS is a float
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    return linkq_run(c, reinterpret_cast<const float2 *>(in), n_frames, frame_stride, frame_len, first_symbol, syms_per_frame, n_points, offset,
                     f_delta, reinterpret_cast<const float2 *>(hk), hk_stride, status, quality);
}

// EXT-8 wide CFO acquisition: one launch of k_cfo_wide over the caller's offset / f_delta / status arrays (include/ofdm_hip.h,
// tests/cfo_wide_ref.py)
static int cfo_wide_run(ofdm_ctx *c, const float2 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len, const int32_t *offset,
                        const int32_t *status, int32_t span, double *f_delta, int32_t *m, float *metric) {
    int rc = cfo_wide_table(c);
    if (rc) return rc;
    CfoWideParams p;
    p.tune = &c->tune; p.trace = &c->trace;
    p.in = in; p.n_frames = n_frames; p.frame_stride = frame_stride; p.frame_len = frame_len;
    p.sym_len = c->S(); p.span = span;
    p.offset = offset; p.status = status; p.f_delta = f_delta;
    p.tw = c->d_tw; p.trn = c->d_trn;
    p.m = m; p.metric = metric;
    HIP_TRY(c, run_cfo_wide(c->prm.n_fft, p, c->stream, c->num_cu));
    return OFDM_OK;
}
int ofdm_cfo_wide_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len, const int32_t *offset,
                        const int32_t *status, int32_t span, double *f_delta, int32_t *m, float *metric) {
    if (!c || n_frames < 0 || frame_len <= 0 || frame_stride < 0) return OFDM_ERR_INVALID;
    if (span < 1 || span > OFDM_CFO_WIDE_MAX_SPAN) return OFDM_ERR_INVALID;
    if (n_frames && (!in || !offset || !f_delta)) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    return cfo_wide_run(c, reinterpret_cast<const float2 *>(in), n_frames, frame_stride, frame_len, offset, status, span, f_delta, m, metric);
}

// EXT-7 soft combining, the stage: one launch of k_llr_combine (include/ofdm_hip.h, tests/combine_ref.py)
int ofdm_llr_combine_batch(ofdm_ctx *c, const int8_t *llr, int64_t n_frames, int32_t n_branches, int64_t llr_stride, int64_t n_llr,
                           const float *quality, const int32_t *status, const int32_t *n_live, int8_t *out, int64_t out_stride,
                           int32_t *weight) {
    if (!c || n_frames < 0 || n_llr < 0 || n_branches < 1 || n_branches > OFDM_COMBINE_MAX_BRANCHES) return OFDM_ERR_INVALID;
    if (llr_stride < n_llr || out_stride < n_llr || (n_frames && (!llr || !out))) return OFDM_ERR_INVALID;
    if (n_llr > 0x7fffffffll - (1 << 13)) return OFDM_ERR_UNSUPPORTED; // the kernel's column indices are ints
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    CombineParams p;
    p.tune = &c->tune; p.trace = &c->trace;
    p.llr = llr; p.n_frames = n_frames; p.llr_stride = llr_stride; p.n_branches = n_branches; p.n_llr = (int)n_llr;
    p.quality = quality; p.status = status; p.n_live = n_live;
    p.out = out; p.out_stride = out_stride; p.weight = weight;
    HIP_TRY(c, run_llr_combine(p, c->num_cu, c->stream));
    return OFDM_OK;
}

// ------------------------------------------------------------------ pipelines
// The argument rules ofdm_tx_encode_batch and ofdm_tx_encode_sc16_batch share; *frame = ofdm_frame_samples(payload_bytes)
static int tx_encode_check(ofdm_ctx *c, const uint8_t *payload, int64_t n_frames, int64_t payload_stride, int32_t payload_bytes, const void *out,
                           int64_t out_stride, int64_t *frame) {
    if (!c || n_frames < 0 || payload_bytes < 0 || payload_stride < 0) return OFDM_ERR_INVALID;
    if (n_frames && (!out || (payload_bytes && !payload))) return OFDM_ERR_INVALID;
    if (n_frames > 1 && payload_stride < payload_bytes) return OFDM_ERR_INVALID; // rows are prefetched for payload_bytes (include/ofdm_hip.h)
    if (c->mode.has(kLayerFcs) && payload_bytes > 0x7fffffff - OFDM_FCS_OVERHEAD) return OFDM_ERR_UNSUPPORTED;
    *frame = ofdm_frame_samples(c, payload_bytes);
    return out_stride < *frame ? OFDM_ERR_INVALID : OFDM_OK;
}
// The rows the frame kernels map: the caller's payload rows, or what the coding layers made of them
struct TxRows { const uint8_t *src; int64_t stride; const int32_t *len; int32_t bytes; };
// The outer layers (kOuter[...], outside-in) and the inner code (conv / LDPC / Hamming) of the context's mode over n_frames payload rows,
// each into its named workspace.  Shared by the fc32 and the sc16 (EXT-10) encode.
static int tx_code_layers(ofdm_ctx *c, int64_t n_frames, TxRows &r) {
    const ModePlan &m = c->mode;
    const uint8_t *src = r.src; int64_t src_stride = r.stride; const int32_t *src_len = r.len;
    int32_t src_bytes = r.bytes;
    int rc;
    for (int i = 0; i < m.n_outer; i++) { // outside-in: the next layer's frame of this layer's rows
        const OuterStage &s = kOuter[m.outer[i]];
        const int64_t coded = outer_coded_bytes(m.outer[i], src_bytes);
        if (coded > 0x7fffffffll) return OFDM_ERR_UNSUPPORTED;
        void *rows, *len;
        if ((rc = ws_get(c, s.tx_rows, (size_t)coded * (size_t)n_frames, &rows))) return rc;
        if ((rc = ws_get(c, s.tx_len, sizeof(int32_t) * (size_t)n_frames, &len))) return rc;
        if (!src_len) len = nullptr; // only ragged rows carry lengths on
        c->trace.add(s.tx_name);
        HIP_TRY(c, s.encode(c, LayerCall{src, n_frames, src_stride, src_bytes, src_len, (uint8_t *)rows, coded, (int32_t *)len, nullptr, nullptr}));
        src = (const uint8_t *)rows; src_stride = coded; src_len = (const int32_t *)len; src_bytes = (int32_t)coded;
    }
    if (m.inner != OFDM_ECC_NONE) { // HAMMING74 and HAMMING74_SOFT transmit the same frames
        const int64_t coded = inner_coded_bytes(m, src_bytes);
        if ((m.conv() || m.ldpc()) && coded > 0x7fffffffll) return OFDM_ERR_UNSUPPORTED; // (payload_bytes = INT32_MAX)
        void *cw, *cl;
        if ((rc = ws_get(c, kWsTxCoded, (size_t)(coded ? coded : 1) * (size_t)n_frames, &cw))) return rc;
        if ((rc = ws_get(c, kWsTxCodedLen, sizeof(int32_t) * (size_t)n_frames, &cl))) return rc;
        if (m.inner == OFDM_ECC_CONV_K7) {
            c->trace.add("k_conv_encode");
            HIP_TRY(c, run_conv_encode(src, n_frames, src_stride, src_len, src_bytes, (uint8_t *)cw, coded, (int32_t *)cl, c->stream));
        } else if (m.rate() >= 0) {
            c->trace.add("k_conv_encode_p");
            HIP_TRY(c, run_conv_encode_p(src, n_frames, src_stride, src_len, src_bytes, m.rate(), kConvLengthBlock, (uint8_t *)cw, coded,
                                         (int32_t *)cl, c->stream));
        } else if (m.ldpc()) { // the code of [u32 LE p][u32 LE ~p] ++ payload, row by row
            LdpcEncodeParams lp;
            lp.in = src; lp.n_frames = n_frames; lp.in_stride = src_stride; lp.n_bytes = src_bytes; lp.in_len = src_len; lp.framed = 1;
            lp.n_cw = coded / kLdpcCodeBytes; lp.out = (uint8_t *)cw; lp.out_stride = coded; lp.out_len = (int32_t *)cl;
            c->trace.add(ldpc_encode_name(m.ldpc_rate()));
            HIP_TRY(c, run_ldpc_encode(lp, m.ldpc_rate(), c->num_cu, &c->tune, c->stream));
        } else {
            HIP_TRY(c, run_ham_encode(src, n_frames, src_stride, src_len, src_bytes, (uint8_t *)cw, coded, (int32_t *)cl, c->stream));
        }
        src = (const uint8_t *)cw; src_stride = coded; src_len = src_len ? (const int32_t *)cl : nullptr;
        src_bytes = (int32_t)coded;
    }
    r = TxRows{src, src_stride, src_len, src_bytes};
    return OFDM_OK;
}
// the frame kernels' arguments for coded rows r of frames laid out for payload_bytes
static SymParams tx_frame_params(ofdm_ctx *c, const TxRows &r, int64_t n_frames, int32_t payload_bytes) {
    SymParams p = base_params(c);
    p.n_frames = n_frames; p.syms_per_frame = (int)ofdm_data_symbols(c, payload_bytes);
    p.payload = r.src; p.payload_stride = r.stride; p.payload_len = r.len; p.payload_bytes = r.bytes;
    return p;
}
// ofdm_tx_encode_batch behind its argument checks: the coding layers, then the frames (the trace is appended to)
static int tx_encode_fc32(ofdm_ctx *c, const uint8_t *payload, int64_t n_frames, int64_t payload_stride, const int32_t *payload_len,
                          int32_t payload_bytes, float2 *out, int64_t out_stride, int64_t frame) {
    TxRows r{payload, payload_stride, payload_len, payload_bytes};
    int rc;
    if ((rc = tx_code_layers(c, n_frames, r))) return rc;
    const int S = c->S();
    SymParams p = tx_frame_params(c, r, n_frames, payload_bytes);
    p.out = out; p.out_stride_s = out_stride;
    // one workgroup per frame, frame built in LDS, single pass over HBM (kernels_n64.hip)
    if (c->prm.n_fft == 64) FAST_PATH(c, c->tune.no_txframe64, run_txframe64(p, c->d_header, c->header_max, c->stream, c->num_cu));
    // R x 64 two-stage kernel, frames built twice: one pass over HBM (kernels_mid.hip)
    if (c->prm.n_fft < 4096) FAST_PATH(c, c->tune.no_mid_kernels, run_txframe_mid(c->prm.n_fft, p, c->d_header, c->header_max, c->stream, c->num_cu));
    // 64 x 64 two-stage kernel, frames built twice: one pass over HBM (kernels_n4096.hip)
    if (c->prm.n_fft == 4096) FAST_PATH(c, c->tune.no_demod4096, run_txframe4096(p, c->d_header, c->header_max, c->stream, c->num_cu));
    void *mx;
    if ((rc = ws_get(c, kWsFrameMax, sizeof(unsigned) * (size_t)n_frames, &mx))) return rc;
    HIP_TRY(c, hipMemsetAsync(mx, 0, sizeof(unsigned) * (size_t)n_frames, c->stream));
    p.frame_max = (unsigned *)mx;
    HIP_TRY(c, run_tx_symbols(c->prm.n_fft, p, c->stream, c->num_cu));
    c->trace.add("k_tx_finish");
    HIP_TRY(c, run_tx_finish(out, n_frames, out_stride, 10 * S, frame, c->d_header, c->header_max, (const unsigned *)mx, c->stream));
    return OFDM_OK;
}
int ofdm_tx_encode_batch(ofdm_ctx *c, const uint8_t *payload, int64_t n_frames, int64_t payload_stride,
                         const int32_t *payload_len, int32_t payload_bytes, ofdm_fc32 *out, int64_t out_stride) {
    int64_t frame = 0;
    const int rc = tx_encode_check(c, payload, n_frames, payload_stride, payload_bytes, out, out_stride, &frame);
    if (rc || !n_frames) return rc;
    EntryScope scope(c);
    return tx_encode_fc32(c, payload, n_frames, payload_stride, payload_len, payload_bytes, reinterpret_cast<float2 *>(out), out_stride, frame);
}

namespace {
// What steps 1 - 4 of the chain leave to the soft finishing kernels (raw: the hard bytes, for the length header)
struct SoftInput { int32_t *offs; double *fd; const int32_t *nsym; const float2 *hk; uint8_t *raw; int64_t raw_stride, body_steps; const float *q; };
} // namespace
// OFDM_ECC_HAMMING74_SOFT decode: the LLR workspace (one frame chunk of LLR rows) never exceeds this
static const int64_t kSoftLlrBytes = 256ll << 20;

// 4s + 5s of the chain, per frame chunk: hard bytes (for the header) and LLRs in one k_sym<llr>, then ONE finishing kernel -- the header
// and the ML decode of the body (k_rx_finish_soft); OFDM_ECC_CONV_K7: k_viterbi_k7, which also needs a survivor slab per resident
// wavefront; OFDM_ECC_CONV_K7F_*: k_viterbi_k7f, which reads the length from its own coded block and may set status;
// OFDM_ECC_LDPC648 / _R23 / _R34 / _R56: k_ldpc_decode / k_ldpc_decode<r23|r34|r56>, which reads the length from its first code word and
// may set status.
// The finishing kernel of frames f0 .. f0 + nf of d over the LLR rows of one chunk (row 0 = frame f0); vp: the Viterbi launch as planned
// for the chunk size (conv modes)
static int soft_finish_chunk(ofdm_ctx *c, const DecodeCall &d, int64_t f0, int64_t nf, const int8_t *llr, int64_t llr_stride,
                             const int32_t *nsym, const uint8_t *raw, int64_t raw_stride, ViterbiParams &vp, long long v_blocks) {
    const ModePlan &m = c->mode;
    const int bps_bytes = c->bytes_per_symbol();
    uint8_t *out = d.out + f0 * d.out_stride;
    if (m.ldpc()) {
        LdpcDecodeParams lp;
        lp.llr = llr; lp.n_frames = nf; lp.llr_stride = llr_stride; lp.max_iter = OFDM_LDPC_MAX_ITER;
        lp.out = out; lp.out_stride = d.out_stride; lp.status_rw = d.status + f0; lp.out_len = d.out_len + f0;
        lp.nsym = nsym; lp.bytes_per_symbol = bps_bytes;
        HIP_TRY(c, run_ldpc_decode(lp, m.ldpc_rate(), c->num_cu, &c->tune, c->stream));
    } else if (m.conv()) {
        vp.n_frames = nf; vp.out = out; vp.raw = raw; vp.status = d.status + f0; vp.nsym = nsym; vp.out_len = d.out_len + f0;
        if (m.rate() < 0) {
            HIP_TRY(c, run_viterbi_k7(vp, v_blocks, c->stream));
        } else {
            const ViterbiFParams vf{vp, m.rate(), d.status + f0}; // (it may set status)
            HIP_TRY(c, run_viterbi_k7f(vf, v_blocks, c->stream));
        }
    } else {
        HIP_TRY(c, run_rx_finish_soft(raw, raw_stride, llr, llr_stride, nf, d.status + f0, nsym, bps_bytes, out, d.out_stride,
                                      d.out_len + f0, c->stream));
    }
    return OFDM_OK;
}
static const char *soft_finish_name(const ModePlan &m) {
    return m.ldpc() ? ldpc_decode_name(m.ldpc_rate()) : !m.conv() ? "k_rx_finish_soft" : m.rate() < 0 ? "k_viterbi_k7" : "k_viterbi_k7f";
}
// The frames of one chunk of the soft chains: the LLR workspace holds at most kSoftLlrBytes of rows whatever n_frames is
static int64_t soft_chunk_frames(const ofdm_ctx *c, int64_t llr_row_bytes, int64_t n_frames) {
    const int64_t chunk = c->tune.soft_chunk_frames > 0 ? c->tune.soft_chunk_frames : kSoftLlrBytes / llr_row_bytes;
    return std::min(std::max<int64_t>(chunk, 1), n_frames);
}
static int rx_finish_soft(ofdm_ctx *c, const DecodeCall &d, const SoftInput &s) {
    const ModePlan &m = c->mode;
    const int N = c->prm.n_fft, bps_bytes = c->bytes_per_symbol();
    const int64_t llr_row = (int64_t)d.max_symbols * c->carriers() * c->prm.modulation;
    const int64_t llr_stride = (llr_row + 15) & ~(int64_t)15;
    const int64_t chunk = soft_chunk_frames(c, llr_stride, d.n_frames);
    void *w_llr;
    int rc;
    if ((rc = ws_get(c, kWsLlr, (size_t)(llr_stride * chunk), &w_llr))) return rc;
    const int8_t *llr = (const int8_t *)w_llr;
    ViterbiParams vp;
    long long v_blocks = 0;
    if (m.conv()) {
        if ((rc = viterbi_survivors(c, chunk, s.body_steps, vp, &v_blocks))) return rc;
        vp.llr = llr; vp.llr_stride = llr_stride; vp.out_stride = d.out_stride;
        vp.raw_stride = s.raw_stride; vp.bytes_per_symbol = bps_bytes;
    }
    const char *name = soft_finish_name(m);
    for (int64_t f0 = 0; f0 < d.n_frames; f0 += chunk) {
        const int64_t nf = d.n_frames - f0 < chunk ? d.n_frames - f0 : chunk;
        const Trace::Mute later(c->trace, f0 > 0); // the dispatch string names what a chunk ran, once
        const int32_t *nsym = s.nsym + f0;
        const uint8_t *raw = s.raw + f0 * s.raw_stride;
        rc = llr_run(c, d.in + f0 * d.frame_stride, nf, d.frame_stride, d.frame_len, 10, d.max_symbols, s.offs + f0, s.fd + f0, nsym,
                     s.hk + f0 * N, N, OFDM_SOFT_LLR_SCALE, (int8_t *)w_llr, llr_stride, s.raw + f0 * s.raw_stride, s.raw_stride,
                     s.q ? s.q + f0 * N : nullptr, N);
        if (rc) return rc;
        c->trace.add(name);
        if ((rc = soft_finish_chunk(c, d, f0, nf, llr, llr_stride, nsym, raw, s.raw_stride, vp, v_blocks))) return rc;
    }
    return OFDM_OK;
}

// The sizes the inner chain derives from max_symbols, and its two argument checks: the output rows hold what the finishing kernel can
// write, and the longest trellis a frame can ask for is one the Viterbi kernels take
struct InnerPlan { int bps_bytes; int64_t raw_bytes, raw_stride, body_max, body_steps; };
static int inner_plan(ofdm_ctx *c, const DecodeCall &d, InnerPlan &ip) {
    const ModePlan &m = c->mode;
    ip.bps_bytes = c->bytes_per_symbol();
    ip.raw_bytes = (int64_t)d.max_symbols * ip.bps_bytes;
    ip.raw_stride = (ip.raw_bytes + 3) & ~(int64_t)3;   // rows of the raw-byte workspace start on dwords (6-byte BPSK symbols: odd counts)
    // rows must hold what k_rx_finish can write: the whole body without an outer code, floor(body / 7) * 4 bytes after
    // Hamming(7,4) decoding, body / 2 - 1 after Viterbi decoding (include/ofdm_hip.h)
    ip.body_max = decode_body_bytes(c, d.max_symbols);
    if (d.out_stride < inner_row_limit(m, ip.body_max)) return OFDM_ERR_INVALID;
    const int f_rate = m.rate();
    // the longest trellis a frame can ask for (framed: the 72-step length block, then a body cut at the end of the capture)
    ip.body_steps = f_rate < 0 ? 4 * ip.body_max
                               : std::max<int64_t>(4 * kConvLengthBlock, conv_max_steps(8 * std::max<int64_t>(ip.body_max - kConvLengthBlock, 0), f_rate));
    if (m.conv() && ip.body_steps > kViterbiMaxSteps) return OFDM_ERR_UNSUPPORTED;
    return OFDM_OK;
}

// Steps 1 + 2 of the chain over the rows of d (ofdm_rx_decode_batch: the frames; ofdm_rx_decode_combine_batch: the branch rows): timing
// and CFO by the context's sync mode, then the trimmed start, the length check and the live symbols.  Leaves d.status, d.metric and,
// in fe, the arrays the kernels behind it index with: the caller's offset / f_delta arrays or the workspace's.
struct FrontEnd { int32_t *offs; double *fd; int32_t *nsym; };
static int rx_front_end(ofdm_ctx *c, const DecodeCall &d, int bps_bytes, FrontEnd &fe) {
    const int64_t n_frames = d.n_frames, frame_stride = d.frame_stride, frame_len = d.frame_len;
    const int32_t max_symbols = d.max_symbols;
    int32_t *const status = d.status, *const offset = d.offset;
    float *const metric = d.metric;
    void *w_dhat, *w_fd, *w_off, *w_nsym;
    int rc;
    if ((rc = ws_get(c, kWsDhat, sizeof(int32_t) * (size_t)n_frames, &w_dhat))) return rc;
    if ((rc = ws_get(c, kWsFdelta, sizeof(double) * (size_t)n_frames, &w_fd))) return rc;
    if ((rc = ws_get(c, kWsOffset, sizeof(int32_t) * (size_t)n_frames, &w_off))) return rc;
    if ((rc = ws_get(c, kWsNsym, sizeof(int32_t) * (size_t)n_frames, &w_nsym))) return rc;
    int32_t *offs = offset ? offset : (int32_t *)w_off;
    double *fd = d.f_delta ? d.f_delta : (double *)w_fd;
    const float2 *x = d.in;
    if (const KnownSync *known = d.known) {
        // 1k. the caller brings the timing: of the one capture (ofdm_rx_decode_long with lag_lo > 0), or of every row with the row's own
        //     length (ofdm_rx_decode_packets: a row cut by the capture's end is zeros from there on, which every kernel behind reads
        //     as pad_chunk's padding under the scalar frame_len)
        if (c->prm.sync_mode != OFDM_SYNC_SCHMIDL_COX) return OFDM_ERR_INVALID;
        if (known->row_dhat) {
            if (!known->row_len || !d.f_delta || !offset) return OFDM_ERR_INVALID;
            c->trace.add("k_rx_prepare_rows");
            HIP_TRY(c, run_rx_prepare_rows(n_frames, known->row_dhat, fd, known->row_len, c->S(), c->prm.sync_backoff, c->prm.cfo_mode,
                                           max_symbols, bps_bytes, status, offs, (int32_t *)w_nsym, c->stream));
        } else {
            if (n_frames != 1) return OFDM_ERR_INVALID;
            c->trace.add("k_set_sync+k_rx_prepare");
            HIP_TRY(c, run_set_sync((int32_t *)w_dhat, fd, metric, known->d_hat, known->f_delta, known->metric, c->stream));
            HIP_TRY(c, run_rx_prepare(n_frames, (const int32_t *)w_dhat, fd, frame_len, c->S(), c->prm.sync_backoff,
                                      c->prm.cfo_mode, max_symbols, bps_bytes, status, offs, (int32_t *)w_nsym, c->stream));
        }
        if (c->prm.cfo_mode == OFDM_CFO_WIDE && (rc = cfo_wide_run(c, x, n_frames, frame_stride, frame_len, offs, status, OFDM_CFO_WIDE_SPAN, fd, nullptr, nullptr))) return rc;
    } else if (c->prm.sync_mode == OFDM_SYNC_REFERENCE) {
        // 1r. the reference's own detector (src/receiver.rs:20-25): cross-correlation with the locking signal, offset =
        //     idx_max - N (= lag - 1), then frequency_correction on chunks 3 and 4 (receiver.rs:39; always |.|)
        if (frame_len > 0x3fffffff) return OFDM_ERR_UNSUPPORTED;
        void *w_x;
        if ((rc = ws_get(c, kWsSearch, xcorr_workspace_bytes(n_frames, frame_len, c->S()), &w_x))) return rc;
        c->trace.add("k_xcorr+k_rx_prepare_ref");
        HIP_TRY(c, run_xcorr(x, n_frames, frame_stride, frame_len, c->d_header, c->S(), w_x, (int32_t *)w_dhat, metric, nullptr, 0,
                             c->num_cu, c->stream));
        // The REPORTED offset may be negative (idx_max - N, quirk Q1; -N for an all-zero capture) and goes to the caller's array
        // only; the kernels below read the workspace copy, which is 0 for every frame whose status is not OFDM_FRAME_OK, so that
        // no fetch can start in front of the capture.
        HIP_TRY(c, run_rx_prepare_ref(n_frames, (const int32_t *)w_dhat, frame_len, c->S(), max_symbols, bps_bytes, status, offset,
                                      (int32_t *)w_off, (int32_t *)w_nsym, c->stream));
        offs = (int32_t *)w_off;
        if (c->prm.cfo_mode == OFDM_CFO_OFF) HIP_TRY(c, hipMemsetAsync(fd, 0, sizeof(double) * (size_t)n_frames, c->stream));
        else { c->trace.add("k_freq_corr"); HIP_TRY(c, run_freq_correction(x + 3 * c->S(), n_frames, frame_stride, c->S(), c->S(), fd, c->stream, offs, status)); }
    } else {
        // 1. timing + CFO: Schmidl-Cox over the repeated preamble (replaces xcorr_fft, src/receiver.rs:20-25,39)
        rc = ofdm_abi_sc_run(c, x, n_frames, frame_stride, frame_len, d.n_lags, (int32_t *)w_dhat, fd, metric);
        if (rc) return rc;
        // 2. trimmed start, length check, live symbols (receiver.rs:21-36)
        c->trace.add("k_rx_prepare");
        HIP_TRY(c, run_rx_prepare(n_frames, (const int32_t *)w_dhat, fd, frame_len, c->S(), c->prm.sync_backoff,
                                  c->prm.cfo_mode, max_symbols, bps_bytes, status, offs, (int32_t *)w_nsym, c->stream));
        // 2w. EXT-8: the offset's whole multiples of 2 pi / S, from the training blocks; every kernel behind reads the same fd
        if (c->prm.cfo_mode == OFDM_CFO_WIDE && (rc = cfo_wide_run(c, x, n_frames, frame_stride, frame_len, offs, status, OFDM_CFO_WIDE_SPAN, fd, nullptr, nullptr))) return rc;
    }
    fe.offs = offs; fe.fd = fd; fe.nsym = (int32_t *)w_nsym;
    return OFDM_OK;
}
// Step 3 of the generic chain over the same rows: the channel estimate from the 5 training blocks into the workspace, denoised under
// OFDM_CHEST_WLS (EXT-5: H' in place of H^)
static int rx_channel_estimate(ofdm_ctx *c, const DecodeCall &d, const FrontEnd &fe, const float2 **hk) {
    const int N = c->prm.n_fft;
    void *w_hk = nullptr;
    int rc;
    if ((rc = ws_get(c, kWsHk, sizeof(float2) * (size_t)N * (size_t)d.n_frames, &w_hk))) return rc;
    SymParams p = rx_params(c, d.in, d.n_frames, d.frame_stride, d.frame_len, fe.offs, fe.fd);
    p.out = (float2 *)w_hk;
    HIP_TRY(c, run_chest(N, p, c->stream, c->num_cu));
    if (c->prm.chest_mode == OFDM_CHEST_WLS && (rc = chest_smooth_run(c, (const float2 *)w_hk, d.n_frames, (float2 *)w_hk))) return rc;
    *hk = (const float2 *)w_hk;
    return OFDM_OK;
}

// The chain of the plan's inner mode into the rows d.out / d.out_stride: the caller's, or the innermost outer layer's workspace
static int rx_decode_inner(ofdm_ctx *c, const DecodeCall &d, const InnerPlan &ip) {
    const ModePlan &m = c->mode;
    const int64_t n_frames = d.n_frames, frame_stride = d.frame_stride, frame_len = d.frame_len, out_stride = d.out_stride;
    const int32_t max_symbols = d.max_symbols;
    uint8_t *const out = d.out;
    int32_t *const out_len = d.out_len, *const status = d.status;
    int rc;
    const int bps_bytes = ip.bps_bytes;
    const int64_t raw_stride = ip.raw_stride, body_steps = ip.body_steps;
    const int ecc = m.inner;
    const int N = c->prm.n_fft;
    void *w_raw = nullptr;
    const float2 *x = d.in;
    if ((rc = ws_get(c, kWsRaw, (size_t)raw_stride * (size_t)n_frames, &w_raw))) return rc;
    FrontEnd fe;
    if ((rc = rx_front_end(c, d, bps_bytes, fe))) return rc;
    int32_t *const offs = fe.offs;
    double *const fd = fe.fd;
    void *const w_nsym = fe.nsym;
    // 3+4. channel estimate from the 5 training blocks and per data symbol CP strip + FFT + equalise + pilot phase +
    //      demap (receiver.rs:44-83).  N = 64: one fused wave-centric kernel; otherwise the generic pair.
    bool fused = false, finished = false;
    const bool soft = m.soft();                               // the fused frame kernels have no LLR epilogue: the generic chain
    const bool wls = c->prm.chest_mode == OFDM_CHEST_WLS;     // ... and take no channel estimate from outside: the generic chain
    if (N == 1024 && !soft && !wls) { // one workgroup per frame: channel estimate kept in registers, 16 x 64 FFT (kernels_rx1024.hip)
        const bool off = c->tune.no_rxframe1024 != 0; // A/B switch
        const SymParams p = rx_params(c, x, n_frames, frame_stride, frame_len, offs, fd, (const int32_t *)w_nsym, (uint8_t *)w_raw, raw_stride);
        // the kernel also parses the length header, truncates and Hamming-decodes into the caller's rows when they are 4-byte aligned
        bool fin = false;
        const int r = fast_path(c, off ? hipErrorNotSupported
                                       : run_rxframe1024(p, nullptr, c->stream, c->num_cu, out, out_stride, out_len, ecc, &fin));
        if (r == OFDM_OK) { fused = true; finished = fin; }
        else if (r != kNextPath) return r;
    }
    if (N == 64 && !soft && !wls) {
        SymParams p = rx_params(c, x, n_frames, frame_stride, frame_len, offs, fd, (const int32_t *)w_nsym, (uint8_t *)w_raw, raw_stride);
        p.syms_per_frame = max_symbols; // (the launcher's "is there room for a whole frame in the capture" test)
        // without an outer code the kernel also parses the length header and writes the payload to its final place
        const bool fin = ecc == OFDM_ECC_NONE && (reinterpret_cast<uintptr_t>(out) & 3) == 0 && (out_stride & 3) == 0;
        void *w_cut;
        if ((rc = ws_get(c, kWsCut, sizeof(int32_t) * (size_t)(n_frames + 4), &w_cut))) return rc;
        const int r = fast_path(c, fin ? run_rxframe64(p, nullptr, c->stream, c->num_cu, out, out_stride, out_len, nullptr, nullptr, (int32_t *)w_cut)
                                       : run_rxframe64(p, nullptr, c->stream, c->num_cu, nullptr, 0, nullptr, nullptr, nullptr, (int32_t *)w_cut));
        if (r == OFDM_OK) { fused = true; finished = fin; }
        else if (r != kNextPath) return r;
    }
    if (!fused) {
        const float2 *hk = nullptr;
        if ((rc = rx_channel_estimate(c, d, fe, &hk))) return rc;
        if (soft) {
            const float *q = nullptr; // EXT-11: the per-bin LLR weights under OFDM_LLRW_NOISE
            if ((rc = rx_noise_weights(c, x, n_frames, frame_stride, frame_len, offs, fd, status, &q))) return rc;
            const SoftInput si{offs, fd, (const int32_t *)w_nsym, hk, (uint8_t *)w_raw, raw_stride, body_steps, q};
            return rx_finish_soft(c, d, si);
        }
        rc = demod_run(c, x, n_frames, frame_stride, frame_len, 10, max_symbols, offs, fd, (const int32_t *)w_nsym,
                       hk, N, (uint8_t *)w_raw, raw_stride, nullptr);
        if (rc) return rc;
    }
    // 5. length header, truncate [, Hamming decode] (receiver.rs:85-95)
    if (!finished) {
        c->trace.add("k_rx_finish");
        HIP_TRY(c, run_rx_finish((const uint8_t *)w_raw, raw_stride, n_frames, status, (const int32_t *)w_nsym, bps_bytes,
                                 ecc, out, out_stride, out_len, c->stream));
    }
    return OFDM_OK;
}

// The decode chain of the context's mode: the inner chain into the innermost outer layer's workspace (dword rows: the fused frame
// kernels and the layer inside write there as they write to a caller's rows), then every outer layer's kernel inside-out over what
// every frame delivered, in place on out_len / status
struct CombineCall { int32_t n_branches; int32_t *branch_status, *weight; float *quality; };
static int rx_decode_combine_inner(ofdm_ctx *c, const DecodeCall &d, const CombineCall &cc, const InnerPlan &ip);
// Everything that refuses a decode call, before anything is launched: the arguments, and per layer the longest row it can be given
// (n_row[i]) against the stride of the rows it writes (stride[i]; stride[n_outer]: the inner chain's).  combine: the call is
// ofdm_rx_decode_combine_batch's
struct DecodePlan { InnerPlan ip; int64_t n_row[2], stride[3]; };
static int rx_decode_plan(ofdm_ctx *c, const DecodeCall &d, const CombineCall *combine, DecodePlan &pl) {
    if (!c || d.n_frames < 0 || d.frame_len <= 0 || d.max_symbols <= 0) return OFDM_ERR_INVALID;
    if (d.n_frames && (!d.in || !d.out || !d.out_len || !d.status)) return OFDM_ERR_INVALID;
    const ModePlan &m = c->mode;
    int64_t row = inner_row_limit(m, decode_body_bytes(c, d.max_symbols));
    for (int i = m.n_outer - 1; i >= 0; i--) { pl.n_row[i] = row; row = outer_row_limit(m.outer[i], row); }
    pl.stride[0] = d.out_stride;
    for (int i = 0; i < m.n_outer; i++) {
        if (pl.n_row[i] > kOuter[m.outer[i]].rx_max_row) return OFDM_ERR_UNSUPPORTED;
        if (pl.stride[i] < outer_row_limit(m.outer[i], pl.n_row[i])) return OFDM_ERR_INVALID;
        pl.stride[i + 1] = (std::max<int64_t>(pl.n_row[i], 4) + 3) & ~(int64_t)3;
    }
    if (m.n_outer && !d.n_frames) return OFDM_OK; // (an empty call of an outer-coded mode is not held to the inner chain's limits)
    if (d.frame_stride <= 0 && (d.n_frames > 1 || (combine && combine->n_branches > 1))) return OFDM_ERR_INVALID;
    DecodeCall inner = d;
    inner.out_stride = pl.stride[m.n_outer];
    int rc;
    if ((rc = inner_plan(c, inner, pl.ip))) return rc;
    // k_llr_combine's column indices are ints
    if (combine && (int64_t)d.max_symbols * c->carriers() * c->prm.modulation > 0x7fffffffll - (1 << 13)) return OFDM_ERR_UNSUPPORTED;
    return OFDM_OK;
}
static int rx_decode_run(ofdm_ctx *c, const DecodeCall &d, const DecodePlan &pl, const CombineCall *combine) {
    const ModePlan &m = c->mode;
    uint8_t *to[3] = {d.out}; // to[i]: where layer i writes; to[n_outer]: the inner chain
    int rc;
    for (int i = 0; i < m.n_outer; i++) {
        void *w_rows;
        if ((rc = ws_get(c, kOuter[m.outer[i]].rx_rows, (size_t)pl.stride[i + 1] * (size_t)d.n_frames, &w_rows))) return rc;
        to[i + 1] = (uint8_t *)w_rows;
    }
    DecodeCall inner = d;
    inner.out = to[m.n_outer]; inner.out_stride = pl.stride[m.n_outer];
    if ((rc = combine ? rx_decode_combine_inner(c, inner, *combine, pl.ip) : rx_decode_inner(c, inner, pl.ip))) return rc;
    for (int i = m.n_outer - 1; i >= 0; i--) {
        const OuterStage &s = kOuter[m.outer[i]];
        c->trace.add(s.rx_name);
        HIP_TRY(c, s.decode(c, LayerCall{to[i + 1], d.n_frames, pl.stride[i + 1], pl.n_row[i], d.out_len, to[i], pl.stride[i], d.out_len, nullptr, d.status}));
    }
    return OFDM_OK;
}
// A decode entry point: the checks, then -- at the same place for every one of them -- the entry scope and the chain
static int rx_decode_entry(ofdm_ctx *c, const DecodeCall &d, const CombineCall *combine = nullptr) {
    DecodePlan pl;
    const int rc = rx_decode_plan(c, d, combine, pl);
    if (rc || !d.n_frames) return rc;
    EntryScope scope(c);
    return rx_decode_run(c, d, pl, combine);
}
int ofdm_abi_rx_decode(ofdm_ctx *c, const DecodeCall &d) {
    DecodePlan pl;
    const int rc = rx_decode_plan(c, d, nullptr, pl);
    return rc || !d.n_frames ? rc : rx_decode_run(c, d, pl, nullptr);
}

int ofdm_rx_decode_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                         int64_t n_lags, int32_t max_symbols, uint8_t *out, int64_t out_stride, int32_t *out_len,
                         int32_t *status, int32_t *offset, double *f_delta, float *metric) {
    return rx_decode_entry(c, DecodeCall{reinterpret_cast<const float2 *>(in), n_frames, frame_stride, frame_len, n_lags, max_symbols, out,
                                         out_stride, out_len, status, offset, f_delta, metric, nullptr});
}

// ------------------------------------------------------------------ EXT-9: sc16 input
int ofdm_sc16_widen(const ofdm_sc16 *in, int64_t n, float scale, ofdm_fc32 *out) {
    if (n < 0 || !sc16_scale_ok(scale) || (n && (!in || !out))) return OFDM_ERR_INVALID;
    sc16_widen_host(&in->re, n, scale, &out->re);
    return OFDM_OK;
}
int ofdm_sc16_narrow(const ofdm_fc32 *in, int64_t n, float scale, ofdm_sc16 *out, int64_t *clipped) {
    if (n < 0 || !sc16_scale_ok(scale) || (n && (!in || !out))) return OFDM_ERR_INVALID;
    const long long k = sc16_narrow_host(&in->re, n, scale, &out->re);
    if (clipped) *clipped = k;
    return OFDM_OK;
}
// the checks both stages share; *work: there is something to launch
static int sc16_stage_check(const ofdm_ctx *c, const void *in, int64_t n_frames, int64_t in_stride, int64_t frame_len, float scale,
                            const void *out, int64_t out_stride, const void *sc_side, bool *work) {
    if (!c || n_frames < 0 || frame_len < 0 || !sc16_scale_ok(scale)) return OFDM_ERR_INVALID;
    if (in_stride < frame_len || out_stride < frame_len) return OFDM_ERR_INVALID;
    *work = n_frames > 0 && frame_len > 0;
    if (*work && (!in || !out || (reinterpret_cast<uintptr_t>(sc_side) & 3))) return OFDM_ERR_INVALID;
    return OFDM_OK;
}
int ofdm_sc16_widen_batch(ofdm_ctx *c, const ofdm_sc16 *in, int64_t n_frames, int64_t in_stride, int64_t frame_len, float scale,
                          ofdm_fc32 *out, int64_t out_stride) {
    bool work = false;
    const int rc = sc16_stage_check(c, in, n_frames, in_stride, frame_len, scale, out, out_stride, in, &work);
    if (rc || !work) return rc;
    EntryScope scope(c);
    Sc16Params p = sc16_params(c, n_frames, frame_len, in_stride, out_stride, scale);
    p.sc_in = reinterpret_cast<const uint32_t *>(in); p.fc_out = reinterpret_cast<float2 *>(out);
    HIP_TRY(c, run_sc16_widen(p, c->num_cu, c->stream));
    return OFDM_OK;
}
int ofdm_sc16_narrow_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_frames, int64_t in_stride, int64_t frame_len, float scale,
                           ofdm_sc16 *out, int64_t out_stride, int32_t *clipped) {
    bool work = false;
    const int rc = sc16_stage_check(c, in, n_frames, in_stride, frame_len, scale, out, out_stride, out, &work);
    if (rc || !n_frames) return rc;
    if (!work && !clipped) return OFDM_OK;
    EntryScope scope(c);
    Sc16Params p = sc16_params(c, n_frames, frame_len, in_stride, out_stride, scale);
    p.fc_in = reinterpret_cast<const float2 *>(in); p.sc_out = reinterpret_cast<uint32_t *>(out); p.clipped = clipped;
    HIP_TRY(c, run_sc16_narrow(p, c->num_cu, c->stream));
    return OFDM_OK;
}

// The widen path of the sc16 receive entry points: frames [f0, f0 + m) of the caller's rows -> kWsSc16, rows of frame_len samples
// ws_stride apart.  ws_stride keeps the parity of the caller's stride, so that the fc32 path sees rows aligned as the caller's
// widened rows would be; the chunk is the host pipe's (auto_chunk, ofdm_host_path.hip): about 48 MB of widened samples.
struct Sc16Chunks {
    int64_t chunk, ws_stride;
    float2 *ws;
};
static int sc16_chunks(ofdm_ctx *c, WsRole role, int64_t n_frames, int64_t frame_stride, int64_t frame_len, Sc16Chunks &k) {
    k.ws_stride = frame_len + ((frame_len ^ frame_stride) & 1);
    int64_t chunk = c->tune.sc16_chunk_frames;
    if (chunk <= 0) {
        chunk = (int64_t)((size_t)48 << 20) / std::max<int64_t>(k.ws_stride * (int64_t)sizeof(float2), 1);
        if (chunk > 4) chunk &= ~(int64_t)3;
    }
    k.chunk = std::min(std::max<int64_t>(chunk, 1), std::max<int64_t>(n_frames, 1));
    void *w;
    const int rc = ws_get(c, role, (size_t)k.chunk * (size_t)k.ws_stride * sizeof(float2), &w);
    k.ws = static_cast<float2 *>(w);
    return rc;
}
static int sc16_widen_chunk(ofdm_ctx *c, const ofdm_sc16 *in, int64_t f0, int64_t m, int64_t frame_stride, int64_t frame_len, float scale,
                            const Sc16Chunks &k) {
    Sc16Params p = sc16_params(c, m, frame_len, frame_stride, k.ws_stride, scale);
    p.sc_in = reinterpret_cast<const uint32_t *>(in + f0 * frame_stride); p.fc_out = k.ws;
    HIP_TRY(c, run_sc16_widen(p, c->num_cu, c->stream));
    return OFDM_OK;
}

int ofdm_rx_demod_sc16_batch(ofdm_ctx *c, const ofdm_sc16 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len, float scale,
                             int32_t first_symbol, int32_t syms_per_frame, const int32_t *offset, const double *f_delta,
                             const ofdm_fc32 *hk, int64_t hk_stride, uint8_t *out, int64_t out_stride, ofdm_fc32 *soft) {
    if (!c || n_frames < 0 || syms_per_frame < 0 || first_symbol < 0 || frame_len <= 0 || !sc16_scale_ok(scale)) return OFDM_ERR_INVALID;
    if (n_frames && syms_per_frame && (!in || !out || (reinterpret_cast<uintptr_t>(in) & 3))) return OFDM_ERR_INVALID;
    if (out_stride < (int64_t)syms_per_frame * c->bytes_per_symbol()) return OFDM_ERR_INVALID;
    if (hk && hk_stride != 0 && hk_stride != c->prm.n_fft) return OFDM_ERR_INVALID;
    if (!n_frames || !syms_per_frame) return OFDM_OK;
    EntryScope scope(c);
    if (c->prm.n_fft == 64) { // the fused kernel reads the int16 pairs itself
        SymParams p = rx_params(c, nullptr, n_frames, frame_stride, frame_len, offset, f_delta, nullptr, out, out_stride);
        p.first_symbol = first_symbol; p.syms_per_frame = syms_per_frame; p.in_sym_stride = c->S(); p.in_skip = c->prm.cp_len;
        p.hk = reinterpret_cast<const float2 *>(hk); p.hk_stride = hk_stride; p.soft = reinterpret_cast<float2 *>(soft);
        FAST_PATH(c, c->tune.no_demod64_sc16 || c->tune.no_fast64,
                  run_demod64_sc16(p, reinterpret_cast<const uint32_t *>(in), scale, c->stream, c->num_cu));
    }
    Sc16Chunks k;
    int rc;
    if ((rc = sc16_chunks(c, kWsSc16, n_frames, frame_stride, frame_len, k))) return rc;
    for (int64_t f0 = 0; f0 < n_frames; f0 += k.chunk) {
        const int64_t m = std::min(k.chunk, n_frames - f0);
        const Trace::Mute later(c->trace, f0 > 0); // the dispatch string names what a chunk ran, once
        if ((rc = sc16_widen_chunk(c, in, f0, m, frame_stride, frame_len, scale, k))) return rc;
        rc = demod_run(c, k.ws, m, k.ws_stride, frame_len, first_symbol, syms_per_frame, offset ? offset + f0 : nullptr,
                       f_delta ? f_delta + f0 : nullptr, nullptr, hk ? reinterpret_cast<const float2 *>(hk) + f0 * hk_stride : nullptr, hk_stride,
                       out + f0 * out_stride, out_stride,
                       soft ? reinterpret_cast<float2 *>(soft) + f0 * (int64_t)syms_per_frame * c->carriers() : nullptr);
        if (rc) return rc;
    }
    return OFDM_OK;
}

int ofdm_rx_decode_sc16_batch(ofdm_ctx *c, const ofdm_sc16 *in, int64_t n_frames, int64_t frame_stride, int64_t frame_len, float scale,
                              int64_t n_lags, int32_t max_symbols, uint8_t *out, int64_t out_stride, int32_t *out_len, int32_t *status,
                              int32_t *offset, double *f_delta, float *metric) {
    if (!c || n_frames < 0 || frame_len <= 0 || max_symbols <= 0 || !sc16_scale_ok(scale)) return OFDM_ERR_INVALID;
    if (n_frames && (!in || !out || !out_len || !status || (reinterpret_cast<uintptr_t>(in) & 3))) return OFDM_ERR_INVALID;
    // the chain's own argument checks, on the call as the widened rows present it (their stride is the workspace's: never refused)
    const DecodeCall all{reinterpret_cast<const float2 *>(in), n_frames, 1, frame_len, n_lags, max_symbols, out, out_stride, out_len, status, offset,
                         f_delta, metric, nullptr};
    DecodePlan pl;
    int rc = rx_decode_plan(c, all, nullptr, pl);
    if (rc || !n_frames) return rc;
    EntryScope scope(c);
    Sc16Chunks k;
    if ((rc = sc16_chunks(c, kWsSc16, n_frames, frame_stride, frame_len, k))) return rc;
    for (int64_t f0 = 0; f0 < n_frames; f0 += k.chunk) {
        const int64_t m = std::min(k.chunk, n_frames - f0);
        const Trace::Mute later(c->trace, f0 > 0); // the dispatch string names what a chunk ran, once
        if ((rc = sc16_widen_chunk(c, in, f0, m, frame_stride, frame_len, scale, k))) return rc;
        const DecodeCall d{k.ws, m, k.ws_stride, frame_len, n_lags, max_symbols, out + f0 * out_stride, out_stride, out_len + f0, status + f0,
                           offset ? offset + f0 : nullptr, f_delta ? f_delta + f0 : nullptr, metric ? metric + f0 : nullptr, nullptr};
        if ((rc = ofdm_abi_rx_decode(c, d))) return rc;
    }
    return OFDM_OK;
}

// ------------------------------------------------------------------ EXT-10: sc16 output
// Row f = ofdm_sc16_narrow(frame f of ofdm_tx_encode_batch, scale).  N = 64 frames of up to 56 data symbols into a 16-byte aligned
// output with rows a multiple of 4 samples apart: the coding layers, then k_txframe64_sc16, which narrows in its store phase.  Everything
// else: the unchanged fc32 encode on a chunk of frames into kWsTxSc16 (rows an even number of samples apart, 16-byte aligned: what the
// fc32 frame kernels like best), then k_sc16_narrow with per-row counts into the caller's rows.
int ofdm_tx_encode_sc16_batch(ofdm_ctx *c, const uint8_t *payload, int64_t n_frames, int64_t payload_stride, const int32_t *payload_len,
                              int32_t payload_bytes, float scale, ofdm_sc16 *out, int64_t out_stride, int32_t *clipped) {
    if (!sc16_scale_ok(scale)) return OFDM_ERR_INVALID;
    int64_t frame = 0;
    int rc = tx_encode_check(c, payload, n_frames, payload_stride, payload_bytes, out, out_stride, &frame);
    if (rc || !n_frames) return rc;
    if (reinterpret_cast<uintptr_t>(out) & 3) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    // the launcher's own envelope (kernels_n64_tx_sc16.hip), asked before the rows are coded: they are coded once on either path
    if (c->prm.n_fft == 64 && !c->tune.no_txframe64_sc16 && !c->tune.no_txframe64 &&
        txframe64_sc16_takes((int)ofdm_data_symbols(c, payload_bytes), out, out_stride)) {
        TxRows r{payload, payload_stride, payload_len, payload_bytes};
        if ((rc = tx_code_layers(c, n_frames, r))) return rc;
        const SymParams p = tx_frame_params(c, r, n_frames, payload_bytes);
        HIP_TRY(c, run_txframe64_sc16(p, c->d_header, c->header_max, reinterpret_cast<uint32_t *>(out), out_stride, scale, clipped, c->stream,
                                      c->num_cu));
        return OFDM_OK;
    }
    Sc16Chunks k;
    if ((rc = sc16_chunks(c, kWsTxSc16, n_frames, 0, frame, k))) return rc;
    for (int64_t f0 = 0; f0 < n_frames; f0 += k.chunk) {
        const int64_t m = std::min(k.chunk, n_frames - f0);
        // Kept on purpose: this path names what its LAST chunk ran, where every other chunk loop names the first
        const Trace::Mute earlier(c->trace, f0 + m < n_frames);
        rc = tx_encode_fc32(c, payload ? payload + f0 * payload_stride : nullptr, m, payload_stride, payload_len ? payload_len + f0 : nullptr,
                            payload_bytes, k.ws, k.ws_stride, frame);
        if (rc) return rc;
        Sc16Params p = sc16_params(c, m, frame, k.ws_stride, out_stride, scale);
        p.fc_in = k.ws; p.sc_out = reinterpret_cast<uint32_t *>(out + f0 * out_stride);
        p.clipped = clipped ? clipped + f0 : nullptr;
        HIP_TRY(c, run_sc16_narrow(p, c->num_cu, c->stream));
    }
    return OFDM_OK;
}

// EXT-7: the inner chain over frames of R captures.  d: the call per FRAME (out, out_len, status), its offset / f_delta / metric per BRANCH
// ROW.  Front end, link quality and LLRs per branch row, k_llr_combine, then the mode's finishing kernel on the combined rows.
// The LLR workspace holds one chunk of frames: R branch rows and the combined row each.
static int rx_decode_combine_inner(ofdm_ctx *c, const DecodeCall &d, const CombineCall &cc, const InnerPlan &ip) {
    const ModePlan &m = c->mode;
    const int R = cc.n_branches, N = c->prm.n_fft;
    int rc;
    const int llr_unit = c->carriers() * c->prm.modulation;
    const int64_t llr_row = (int64_t)d.max_symbols * llr_unit;
    const int64_t rows = d.n_frames * R;
    void *w_bst = nullptr, *w_q = nullptr, *w_ns, *w_llr;
    if (!cc.branch_status && (rc = ws_get(c, kWsBranchStatus, sizeof(int32_t) * (size_t)rows, &w_bst))) return rc;
    if (!cc.quality && (rc = ws_get(c, kWsBranchQuality, sizeof(float) * kQualityFields * (size_t)rows, &w_q))) return rc;
    if ((rc = ws_get(c, kWsCombinedNsym, sizeof(int32_t) * (size_t)d.n_frames, &w_ns))) return rc;
    int32_t *const bst = cc.branch_status ? cc.branch_status : (int32_t *)w_bst;
    float *const quality = cc.quality ? cc.quality : (float *)w_q;
    // 1. the front end over the branch rows
    DecodeCall b = d;
    b.n_frames = rows; b.out = nullptr; b.out_len = nullptr; b.status = bst;
    FrontEnd fe;
    if ((rc = rx_front_end(c, b, ip.bps_bytes, fe))) return rc;
    const float2 *hk = nullptr;
    if ((rc = rx_channel_estimate(c, b, fe, &hk))) return rc;
    // 2. link quality from the training blocks
    if ((rc = linkq_run(c, b.in, rows, b.frame_stride, b.frame_len, 10, 0, nullptr, fe.offs, fe.fd, hk, N, bst, quality))) return rc;
    const float *q = nullptr; // EXT-11: the per-bin LLR weights of every branch row under OFDM_LLRW_NOISE
    if ((rc = rx_noise_weights(c, b.in, rows, b.frame_stride, b.frame_len, fe.offs, fe.fd, bst, &q))) return rc;
    // 3 - 5. per chunk of frames: LLRs of the branch rows, the combined rows behind them, the finishing kernel
    const int64_t llr_stride = (llr_row + 15) & ~(int64_t)15;
    const int64_t chunk = soft_chunk_frames(c, llr_stride, d.n_frames);
    if ((rc = ws_get(c, kWsLlr, (size_t)(llr_stride * chunk) * (size_t)(R + 1), &w_llr))) return rc;
    int8_t *const branch_llr = (int8_t *)w_llr, *const combined = branch_llr + llr_stride * chunk * R;
    ViterbiParams vp;
    long long v_blocks = 0;
    if (m.conv()) {
        if ((rc = viterbi_survivors(c, chunk, ip.body_steps, vp, &v_blocks))) return rc;
        vp.llr = combined; vp.llr_stride = llr_stride; vp.out_stride = d.out_stride;
        vp.raw_stride = 0; vp.bytes_per_symbol = ip.bps_bytes;
    }
    for (int64_t f0 = 0; f0 < d.n_frames; f0 += chunk) {
        const int64_t nf = d.n_frames - f0 < chunk ? d.n_frames - f0 : chunk, r0 = f0 * R;
        const Trace::Mute later(c->trace, f0 > 0); // the dispatch string names what a chunk ran, once
        rc = llr_run(c, b.in + r0 * b.frame_stride, nf * R, b.frame_stride, b.frame_len, 10, d.max_symbols, fe.offs + r0, fe.fd + r0, fe.nsym + r0,
                     hk + r0 * N, N, OFDM_SOFT_LLR_SCALE, branch_llr, llr_stride, nullptr, 0, q ? q + r0 * N : nullptr, N);
        if (rc) return rc;
        CombineParams p;
        p.tune = &c->tune; p.trace = &c->trace;
        p.llr = branch_llr; p.n_frames = nf; p.llr_stride = llr_stride; p.n_branches = R; p.n_llr = (int)llr_row;
        p.quality = quality + r0 * kQualityFields; p.status = bst + r0; p.n_live = fe.nsym + r0; p.live_unit = llr_unit;
        p.out = combined; p.out_stride = llr_stride; p.weight = cc.weight ? cc.weight + r0 : nullptr;
        p.status_out = d.status + f0; p.nsym_out = (int32_t *)w_ns + f0;
        HIP_TRY(c, run_llr_combine(p, c->num_cu, c->stream));
        c->trace.add(soft_finish_name(m));
        // (the framed Viterbi kernel takes chain mode from its status array; no mode supported here reads hard bytes: raw = nullptr)
        if ((rc = soft_finish_chunk(c, d, f0, nf, combined, llr_stride, (const int32_t *)w_ns + f0, nullptr, 0, vp, v_blocks))) return rc;
    }
    return OFDM_OK;
}

int ofdm_rx_decode_combine_batch(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_frames, int32_t n_branches, int64_t frame_stride, int64_t frame_len,
                                 int64_t n_lags, int32_t max_symbols, uint8_t *out, int64_t out_stride, int32_t *out_len, int32_t *status,
                                 int32_t *branch_status, int32_t *offset, double *f_delta, float *metric, int32_t *weight, float *quality) {
    if (!c || n_branches < 1 || n_branches > OFDM_COMBINE_MAX_BRANCHES) return OFDM_ERR_INVALID;
    // the inner code must read nothing from one capture's hard bytes: the framed convolutional modes and the LDPC modes
    if (!(c->mode.rate() >= 0 || c->mode.ldpc())) return OFDM_ERR_UNSUPPORTED;
    const DecodeCall d{reinterpret_cast<const float2 *>(in), n_frames, frame_stride, frame_len, n_lags, max_symbols, out, out_stride, out_len,
                       status, offset, f_delta, metric, nullptr};
    const CombineCall cc{n_branches, branch_status, weight, quality};
    return rx_decode_entry(c, d, &cc);
}

// ---- EXT-13: every packet of one long capture in one batched decode (include/ofdm_hip.h; tests/packets_ref.py)
// The gathered rows of one chunk never exceed this (at least one row a chunk)
static const int64_t kPacketRowsBytes = 256ll << 20;
static const int64_t kPacketsMaxSamples = (int64_t)1 << 40; // ofdm_sc_scan_long's bound: what the 64-bit sample indices are held to

int ofdm_abi_rx_decode_packets(ofdm_ctx *c, const float2 *in, int64_t n, int64_t n_det, const int64_t *d_hat, const double *f_delta,
                               const float *metric, int32_t max_symbols, uint8_t *out, int64_t out_stride, int32_t *out_len, int32_t *status,
                               int64_t *offset, double *f_delta_out, float *metric_out, int64_t n_whole) {
    const int S = c->S();
    // (n_whole > n: `in` is the tail of a capture of n_whole samples -- a stream's window -- and the rows get the length that capture's rows have)
    const int64_t R = std::min<int64_t>((10 + (int64_t)max_symbols) * S + 2, (std::max(n, n_whole) + 1) & ~(int64_t)1);
    int64_t chunk = c->tune.packets_chunk_rows > 0 ? c->tune.packets_chunk_rows : kPacketRowsBytes / (R * (int64_t)sizeof(float2));
    chunk = std::min(std::max<int64_t>(chunk, 1), n_det);
    const size_t nd = (size_t)n_det;
    void *w_det, *w_geom, *w_rows, *w_fd = nullptr, *w_off;
    int rc;
    if ((rc = ws_get(c, kWsPktDet, PktDetections(nullptr, nd).bytes + 16, &w_det))) return rc;
    if ((rc = ws_get(c, kWsPktGeom, PktGeometry(nullptr, nd).bytes + 16, &w_geom))) return rc;
    if ((rc = ws_get(c, kWsPktRows, (size_t)chunk * (size_t)R * sizeof(float2) + 256, &w_rows))) return rc;
    if (!f_delta_out && (rc = ws_get(c, kWsPktFdelta, nd * sizeof(double), &w_fd))) return rc;
    if ((rc = ws_get(c, kWsPktOffset, nd * sizeof(int32_t), &w_off))) return rc;
    PktParams p;
    p.tune = &c->tune; p.trace = &c->trace;
    p.in = in; p.n = n; p.n_det = n_det; p.R = R; p.L = S; p.backoff = c->prm.sync_backoff;
    const PktDetections up(w_det, nd);
    const PktGeometry geom(w_geom, nd);
    p.d_hat = up.d_hat; p.f_delta_in = up.f_delta; p.metric_in = up.metric;
    p.row_start = geom.row_start; p.row_dhat = geom.row_dhat; p.row_len = geom.row_len;
    p.f_delta = f_delta_out ? f_delta_out : static_cast<double *>(w_fd);
    p.metric = metric_out;
    p.rows = static_cast<float2 *>(w_rows);
    HIP_TRY(c, hipMemcpyAsync(up.d_hat, d_hat, nd * sizeof(*d_hat), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(up.f_delta, f_delta, nd * sizeof(*f_delta), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(up.metric, metric, nd * sizeof(*metric), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, run_pkt_rows(p, c->stream));
    int32_t *row_off = static_cast<int32_t *>(w_off);
    for (int64_t k0 = 0; k0 < n_det; k0 += chunk) {
        const int64_t m = std::min(chunk, n_det - k0);
        const Trace::Mute later(c->trace, k0 > 0); // the dispatch string names what a chunk ran, once
        p.row0 = k0; p.n_rows = m;
        HIP_TRY(c, run_gather_rows(p, c->num_cu, c->stream));
        if (c->tune.packets_gather_only) continue; // laboratory key: the gather's time on its own, nothing is delivered
        const KnownSync k{0, 0.0, 0.f, p.row_dhat + k0, p.row_len + k0};
        const DecodeCall d{p.rows, m, R, R, 0, max_symbols, out + k0 * out_stride, out_stride, out_len + k0, status + k0, row_off + k0,
                           p.f_delta + k0, nullptr, &k};
        if ((rc = ofdm_abi_rx_decode(c, d))) return rc;
    }
    if (offset && !c->tune.packets_gather_only) {
        c->trace.add("k_pkt_finish");
        HIP_TRY(c, run_pkt_finish(n_det, p.row_start, row_off, status, reinterpret_cast<long long *>(offset), c->stream));
    }
    return OFDM_OK;
}

int ofdm_rx_decode_packets(ofdm_ctx *c, const ofdm_fc32 *in_dev, int64_t n_samples, int64_t n_det, const int64_t *d_hat, const double *f_delta,
                           const float *metric, int32_t max_symbols, uint8_t *out_dev, int64_t out_stride, int32_t *out_len_dev,
                           int32_t *status_dev, int64_t *offset_dev, double *f_delta_dev, float *metric_dev) {
    if (!c || n_det < 0 || n_samples < 0 || max_symbols <= 0) return OFDM_ERR_INVALID;
    if (n_det && (!in_dev || !d_hat || !f_delta || !metric || !out_dev || !out_len_dev || !status_dev)) return OFDM_ERR_INVALID;
    if (c->prm.sync_mode != OFDM_SYNC_SCHMIDL_COX || n_samples > kPacketsMaxSamples || n_det > 0x7fffffff) return OFDM_ERR_UNSUPPORTED;
    for (int64_t k = 0; k < n_det; k++)
        if (d_hat[k] < 0 || d_hat[k] >= n_samples) return OFDM_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(in_dev) & 7) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    if (!n_det) return OFDM_OK;
    // (the row-size rule of ofdm_rx_decode_batch is checked by the chain before its first launch, but behind the upload: check it here)
    if (out_stride < decode_row_bytes(c, max_symbols)) return OFDM_ERR_INVALID;
    return ofdm_abi_rx_decode_packets(c, reinterpret_cast<const float2 *>(in_dev), n_samples, n_det, d_hat, f_delta, metric, max_symbols, out_dev,
                                      out_stride, out_len_dev, status_dev, offset_dev, f_delta_dev, metric_dev, 0);
}

// CHANNEL (src/channel.rs:26-31): 64 taps, the non-zero ones are 8..16 and 18
static const double kChannelTaps[64] = {
    0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -0.0000, -0.1912, 0.9316, 0.2821, -0.1990, 0.1630, -0.1017, 0.0544, -0.0261,
    0.0090, 0.0000, -0.0034};

int ofdm_channel_taps(double *taps64) {
    if (!taps64) return OFDM_ERR_INVALID;
    for (int i = 0; i < 64; i++) taps64[i] = kChannelTaps[i];
    return OFDM_OK;
}

int ofdm_channel_batch(ofdm_ctx *c, const ofdm_fc32 *tx, int64_t n_frames, int64_t tx_stride, int64_t tx_len, double snr_db,
                       int32_t timing_error, uint64_t seed, const int32_t *delay, const double *f_delta_in, ofdm_fc32 *out,
                       int64_t out_stride, int64_t out_len, double *f_delta_out) {
    if (!c || n_frames < 0 || tx_len <= 0 || tx_stride < 0 || out_len < tx_len + 63 || out_stride < out_len) return OFDM_ERR_INVALID;
    if (n_frames && (!tx || !out)) return OFDM_ERR_INVALID;
    if (n_frames > 1 && tx_stride <= 0) return OFDM_ERR_INVALID;
    if (!(snr_db == snr_db)) return OFDM_ERR_INVALID;
    if (!n_frames) return OFDM_OK;
    EntryScope scope(c);
    ChannelParams p;
    p.tx = reinterpret_cast<const float2 *>(tx); p.n_frames = n_frames; p.tx_stride = tx_stride; p.tx_len = tx_len;
    p.snr_lin = std::pow(10.0, snr_db / 10.0); // channel.rs:40
    p.timing_error = timing_error != 0; p.seed = seed; p.delay = delay; p.f_delta_in = f_delta_in;
    p.out = reinterpret_cast<float2 *>(out); p.out_stride = out_stride; p.out_len = out_len; p.f_delta_out = f_delta_out;
    for (int i = 0; i < 64; i++)
        if (kChannelTaps[i] != 0.0 && p.n_taps < 16) { p.tap_idx[p.n_taps] = i; p.tap_val[p.n_taps] = (float)kChannelTaps[i]; p.n_taps++; }
    HIP_TRY(c, run_channel(p, c->num_cu, c->stream));
    return OFDM_OK;
}

int ofdm_hbm_read_probe(ofdm_ctx *c, const ofdm_fc32 *in, int64_t n_symbols, int32_t pattern) {
    if (!c || n_symbols < 0 || pattern < 0 || pattern > 2 || (n_symbols && !in)) return OFDM_ERR_INVALID;
    EntryScope scope(c);
    void *sink;
    int rc = ws_get(c, kWsProbeSink, 64, &sink);
    if (rc) return rc;
    HIP_TRY(c, run_read_probe(reinterpret_cast<const float2 *>(in), n_symbols, pattern, (unsigned *)sink, c->num_cu, c->stream));
    return OFDM_OK;
}

int ofdm_timer_start(ofdm_ctx *c) {
    if (!c) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    return OFDM_OK;
}
int ofdm_timer_stop_ms(ofdm_ctx *c, float *ms) {
    if (!c || !ms) return OFDM_ERR_INVALID;
    DeviceGuard dev_guard(c->device);
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->ev1));
    HIP_TRY(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return OFDM_OK;
}

} // extern "C"
