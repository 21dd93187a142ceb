// Short damaged runs mended in place by least-squares autoregressive interpolation (si_mend_runs).
//
// One workgroup per row (start s, length m) of the run table the detectors emit; p = order, K = context, e = s + m.  A row's status is
// the first that applies: 6 BADROW (s < 0, m < 1, e > n), 0 LONG (m > max_len), 3 EDGE (s - K < 0 or e + K > n), 4 NEAR (row i - 1 ends
// past s - K or row i + 1 starts before e + K), 5 NONFINITE (a non-finite context sample, or a non-finite result), 1 AR, 2 LINE.
//
// WRITE SET.  Only AR and LINE write, and they write only the samples [s, e) of the one channel -- the sample's own 4, 2 or 3 bytes --
// and the row's status word; every other status writes its status word alone, and BADROW reads no sample.  Nothing of [s, e) is stored
// before the whole solve has succeeded and every result was found finite.
// READ SET.  A row that passed NEAR reads [s - K, s) and [e, e + K) of its channel, never [s, e), and rows i - 1 and i + 1 of the table.
// On a sorted, disjoint table NEAR makes those 2 K samples disjoint from every other row's [s', e'): no workgroup reads what another
// writes, so the result does not depend on scheduling, and a row alone gives the bytes of the same row inside a table.
// No atomics; every sum is taken by one thread in one fixed order, so the same input gives the same bits on every call.
//
// LDS: the window as float64 (2 K + m <= 2112 values, 16.5 KB), the m x m factor (64 rows of 65, 32.5 KB), the autocorrelation partials
// and the vectors: 54 KB, static.  Every __syncthreads() is reached by all 256 threads: what a branch around one tests is read from the
// table or from a word of LDS behind a barrier, the same for the whole workgroup.  Nothing here is tuned for speed.
#include "common.h"

#pragma clang fp contract(off)                      // the float64 expressions as written: a * b + c rounds twice, as the reference does

namespace {

constexpr int MD_THREADS = 256;
constexpr int MD_MAX_LEN = SI_MEND_MAX_LEN, MD_MAX_ORDER = SI_MEND_MAX_ORDER, MD_MAX_CTX = SI_MEND_MAX_CONTEXT;
constexpr int MD_LD = MD_MAX_LEN + 1;               // the factor's row stride
constexpr int MD_PARTS = 8;                         // partial sums per lag
static_assert((2 * MD_MAX_CTX + MD_MAX_LEN + MD_MAX_LEN * MD_LD + (MD_MAX_ORDER + 1) * (MD_PARTS + 3) + 2 * MD_MAX_LEN) * 8 + 16 <= 64 * 1024,
              "the static LDS of mend_runs_kernel");

__device__ __forceinline__ double md_value(float v) { return (double)v; }
__device__ __forceinline__ double md_value(int16_t v) { return (double)v; }
__device__ __forceinline__ double md_value(SiS24 v) { return (double)v.value(); }
__device__ __forceinline__ bool md_finite(float v) { return __builtin_fabsf(v) <= __FLT_MAX__; }
__device__ __forceinline__ bool md_finite(int16_t) { return true; }
__device__ __forceinline__ bool md_finite(SiS24) { return true; }

// would u be stored as a finite sample?  fp32: after the rounding to float; PCM: before the clamp
__device__ __forceinline__ bool md_result_finite(const float*, double u) { return __builtin_fabsf((float)u) <= __FLT_MAX__; }
__device__ __forceinline__ bool md_result_finite(const int16_t*, double u) { return __builtin_fabs(u) <= __DBL_MAX__; }
__device__ __forceinline__ bool md_result_finite(const SiS24*, double u) { return __builtin_fabs(u) <= __DBL_MAX__; }

// fp32 stores (float) u; PCM stores rint(u), ties to even, clamped to the type's range, as the sample's own bytes
__device__ __forceinline__ double md_round_clamp(double u, double lo, double hi) { const double r = __builtin_rint(u); return r < lo ? lo : r > hi ? hi : r; }
__device__ __forceinline__ void md_store(float* p, double u) { *p = (float)u; }
__device__ __forceinline__ void md_store(int16_t* p, double u) { *p = (int16_t)(int)md_round_clamp(u, -32768.0, 32767.0); }
__device__ __forceinline__ void md_store(SiS24* p, double u) { *p = SiS24((int)md_round_clamp(u, -8388608.0, 8388607.0)); }

template <class T>
__global__ __launch_bounds__(MD_THREADS) void mend_runs_kernel(T* __restrict__ x, int n, int ch, int channel, const int32_t* __restrict__ runs,
                                                               int n_runs, int max_len, int p, int K, int32_t* __restrict__ status) {
    __shared__ double w[2 * MD_MAX_CTX + MD_MAX_LEN];
    __shared__ double fac[MD_MAX_LEN * MD_LD];
    __shared__ double part[(MD_MAX_ORDER + 1) * MD_PARTS];
    __shared__ double r[MD_MAX_ORDER + 1], a[MD_MAX_ORDER + 1], b[MD_MAX_ORDER + 1], d[MD_MAX_LEN], u[MD_MAX_LEN];
    __shared__ int line_flag;
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= n_runs) return;

    // ---- the row's status from the table alone: the same words in every thread, so the exit is the whole workgroup's
    const long s = runs[2 * row], m = runs[2 * row + 1], e = s + m;
    int st = -1;
    if (s < 0 || m < 1 || e > n) st = SI_MEND_BADROW;
    else if (m > max_len) st = SI_MEND_LONG;
    else if (s - K < 0 || e + K > n) st = SI_MEND_EDGE;
    else {
        bool near = false;
        if (row > 0) near = (long)runs[2 * row - 2] + (long)runs[2 * row - 1] > s - K;
        if (row + 1 < n_runs) near = near || (long)runs[2 * row + 2] < e + K;
        if (near) st = SI_MEND_NEAR;
    }
    if (st >= 0) {
        if (tid == 0) status[row] = st;
        return;
    }

    // ---- the window x[s - K .. e + K) of the channel as float64; [K, K + M) is not read.  0 <= s - K and e + K <= n were checked above.
    const int M = (int)m, W = 2 * K + M;
    T* const xw = x + ((s - K) * (long)ch + channel);
    int bad = 0;
    for (int t = tid; t < W; t += MD_THREADS) {
        double v = 0.0;
        if (t < K || t >= K + M) {
            const T raw = xw[(long)t * ch];
            bad |= !md_finite(raw);
            v = md_value(raw);
        }
        w[t] = v;
    }
    if (tid == 0) line_flag = 0;
    if (__syncthreads_or(bad)) {
        if (tid == 0) status[row] = SI_MEND_NONFINITE;
        return;
    }

    // ---- r[k], k = 0 .. p: the products of each side alone, MD_PARTS interleaved partial sums per lag, each by one thread in index order
    for (int task = tid; task < (p + 1) * MD_PARTS; task += MD_THREADS) {
        const int k = task / MD_PARTS, sub = task % MD_PARTS;
        double acc = 0.0;
        for (int t = sub; t + k < K; t += MD_PARTS) acc += w[t] * w[t + k];
        for (int t = K + M + sub; t + k < W; t += MD_PARTS) acc += w[t] * w[t + k];
        part[task] = acc;
    }
    __syncthreads();

    // ---- Levinson-Durbin, one thread
    if (tid == 0) {
        for (int k = 0; k <= p; ++k) {
            double acc = part[k * MD_PARTS];
            for (int q = 1; q < MD_PARTS; ++q) acc += part[k * MD_PARTS + q];
            r[k] = acc;
        }
        r[0] = r[0] * (1.0 + 1e-9);
        int line = 0;
        if (r[0] == 0.0) line = 1;
        else {
            double E = r[0];
            a[0] = 1.0;
            for (int i = 1; i <= p; ++i) {
                double acc = r[i];
                for (int j = 1; j < i; ++j) acc += a[j] * r[i - j];
                const double kap = -acc / E;
                for (int j = 1; 2 * j <= i; ++j) {
                    const double lo = a[j] + kap * a[i - j], hi = a[i - j] + kap * a[j];
                    a[j] = lo;
                    a[i - j] = hi;
                }
                a[i] = kap;
                E = E * (1.0 - kap * kap);
                if (!(E > 0.0) || !(E <= __DBL_MAX__)) { line = 1; break; }
            }
        }
        line_flag = line;
    }
    __syncthreads();
    int line = line_flag;

    if (!line) {
        // ---- b[k] = sum_j a_j a_{j + k}
        if (tid <= p) {
            double acc = 0.0;
            for (int j = 0; j + tid <= p; ++j) acc += a[j] * a[j + tid];
            b[tid] = acc;
        }
        __syncthreads();
        // ---- B (banded Toeplitz, stored whole) and d from the known samples within p of each unknown
        for (int idx = tid; idx < M * M; idx += MD_THREADS) {
            const int i = idx / M, j = idx % M, df = i > j ? i - j : j - i;
            fac[i * MD_LD + j] = df <= p ? b[df] : 0.0;
        }
        if (tid < M) {
            const int c = K + tid;
            const int t0 = c - p > 0 ? c - p : 0, t1 = c + p < W - 1 ? c + p : W - 1;
            double acc = 0.0;
            for (int t = t0; t <= t1; ++t)
                if (t < K || t >= K + M) acc += b[t > c ? t - c : c - t] * w[t];
            d[tid] = -acc;
        }
        __syncthreads();
        // ---- Cholesky, column by column: the pivot by one thread, the column below it one element per thread
        for (int j = 0; j < M; ++j) {
            if (tid == 0) {
                double piv = fac[j * MD_LD + j];
                for (int k = 0; k < j; ++k) piv -= fac[j * MD_LD + k] * fac[j * MD_LD + k];
                if (!(piv > 0.0)) line_flag = 1;
                else fac[j * MD_LD + j] = __builtin_sqrt(piv);
            }
            __syncthreads();
            if (line_flag) break;                                   // read behind the barrier: the whole workgroup leaves here
            const double dj = fac[j * MD_LD + j];
            for (int i = j + 1 + tid; i < M; i += MD_THREADS) {
                double v = fac[i * MD_LD + j];
                for (int k = 0; k < j; ++k) v -= fac[i * MD_LD + k] * fac[j * MD_LD + k];
                fac[i * MD_LD + j] = v / dj;
            }
            __syncthreads();
        }
        line = line_flag;
        // ---- L y = d, then L^T u = y, one thread
        if (!line && tid == 0) {
            for (int i = 0; i < M; ++i) {
                double v = d[i];
                for (int k = 0; k < i; ++k) v -= fac[i * MD_LD + k] * u[k];
                u[i] = v / fac[i * MD_LD + i];
            }
            for (int i = M - 1; i >= 0; --i) {
                double v = u[i];
                for (int k = i + 1; k < M; ++k) v -= fac[k * MD_LD + i] * u[k];
                u[i] = v / fac[i * MD_LD + i];
            }
        }
    }
    // ---- the degenerate model: the straight line from x[s - 1] to x[e]
    if (line && tid < M) {
        const double xa = w[K - 1], xb = w[K + M];
        u[tid] = xa + ((double)(tid + 1) / (double)(M + 1)) * (xb - xa);
    }
    __syncthreads();

    // ---- nothing is stored unless every result is finite
    const bool nonfinite = tid < M && !md_result_finite(static_cast<const T*>(nullptr), u[tid]);
    if (__syncthreads_or(nonfinite)) {
        if (tid == 0) status[row] = SI_MEND_NONFINITE;
        return;
    }
    if (tid < M) md_store(xw + (long)(K + tid) * ch, u[tid]);
    if (tid == 0) status[row] = line ? SI_MEND_LINE : SI_MEND_AR;
}

}  // namespace

// The caller (si_mend_runs) checked every argument: 1 <= ch <= SI_MAX_CHANNELS, 0 <= channel < ch, the limits of max_len / order / context.
int si_launch_mend_runs(si_ctx* ctx, void* x, int fmt, int n, int ch, int channel, const int32_t* runs, int n_runs, int max_len, int order,
                        int context, int32_t* status, hipStream_t st) {
    if (n_runs <= 0) return SI_OK;
    const double W = 2.0 * context + max_len;
    si_prof_begin(ctx, "patch_rate", (double)n_runs * (2.0 * (order + 1) * 2.0 * context + 2.0 * max_len * max_len * max_len / 3.0),
                  (double)n_runs * (W * si_sample_bytes(fmt) + 12.0), st);
    si_with_sample(fmt, [&](auto tag) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(tag)>>;
        mend_runs_kernel<T><<<dim3(n_runs), MD_THREADS, 0, st>>>(static_cast<T*>(x), n, ch, channel, runs, n_runs, max_len, order, context, status);
    });
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}
