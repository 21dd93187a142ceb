// rate_kernels.hip -- repair at the file's own sample rate, gfx950: the generated audio of the gaps carried from the
// generator's 22.05 kHz axis to the FILE's rate and blended into the file's own samples, fp32, int16 or packed 24-bit as they lie in the file.
//   patch_rate_kernel<T, INTER>   per touched chunk of 2048 file samples: band-limited interpolation of the window rows at the exact
//                                 rational time i Q / P (si_wings, common.h) + patch_regions_kernel's blend, written into the caller's copy
// T = float | int16_t | SiS24: the file's sample type.  INTER: the chunk is written into one channel of an INTERLEAVED file (DESIGN.md
// 4.18); the mono instantiation folds ch = 1, channel = 0 in.  One body, one __global__ template, one launcher.
// It stands where `resample(patched, 22050, sr)` over the whole repaired recording would: that pass costs every sample of the file a
// 2 x 65-tap float64 sum and returns none of the samples its owner recorded; this one computes the few hundred thousand samples the
// cross-fades and gaps cover and leaves every other sample of `out` alone.
#include "common.h"

constexpr int RK_CHUNK = 2048;      // FILE samples per workgroup: patch_kernels.hip's PC_CHUNK, gaps.region_chunks' chunk

// pc_pcm16's arithmetic (patch_kernels.hip; I_ea/predict.py:204-206): `* 32768`, truncated toward zero, 32768.0 -> 32767, NaN -> 0
__device__ __forceinline__ short rk_pcm16(float v) {
    const float p = v * 32768.0f;
    return (short)(int)fminf(fmaxf(truncf(p == p ? p : 0.f), -32768.f), 32767.f);
}
__device__ __forceinline__ float rk_load(const float* p) { return *p; }
__device__ __forceinline__ float rk_load(const int16_t* p) { return (float)*p * (1.0f / 32768.0f); }     // exact: 16 bits x 2^-15
__device__ __forceinline__ void rk_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void rk_store(int16_t* p, float v) { *p = rk_pcm16(v); }
// Packed 24-bit PCM: rk_pcm16's statement at 24 bits -- `* 8388608`, truncated toward zero, 8388608.0 -> 8388607, NaN -> 0.
// The load is exact (24 bits x 2^-23); the store writes the sample's own three bytes, one byte each: no word a neighbour owns is touched.
__device__ __forceinline__ int rk_pcm24(float v) {
    const float p = v * 8388608.0f;
    return (int)fminf(fmaxf(truncf(p == p ? p : 0.f), -8388608.f), 8388607.f);
}
__device__ __forceinline__ float rk_load(const SiS24* p) { return (float)p->value() * (1.0f / 8388608.0f); }
__device__ __forceinline__ void rk_store(SiS24* p, float v) {
    const int q = rk_pcm24(v);
    p->b[0] = (uint8_t)q;
    p->b[1] = (uint8_t)(q >> 8);
    p->b[2] = (uint8_t)(q >> 16);
}

// grid (Q), 256 threads, rt.row_cap floats of dynamic LDS.  Workgroup q owns file samples [c0, c1) of chunk rt.chunk[q] and walks spans
// [k0[q], k1[q]) -- q is workgroup-uniform, so the whole table arrives through scalar loads and the span loop is uniform.  Per span ks
// that meets the chunk in [ia, ib):
//   stage   the 22.05 kHz samples its interpolation reads, [floor(ia Q / P) - H, floor((ib - 1) Q / P) + H], from the span's window row
//           into LDS: lane t loads element t, t + 256, ... (coalesced whatever the row's alignment -- rows start at arbitrary samples);
//           samples before recording sample 0 and at / past the window's win_lim become zeros here, as the resampler treats a clip's ends.
//           ib - ia <= 2048, so the range holds at most floor(2047 Q / P) + 2 + 2 H = row_cap samples (P / Q = (sr, 22050) / gcd).
//   weight  per sample m of [ia, ib): patch_regions_kernel's walk over ALL the chunk's spans -- the maximum of rise / 1 / mirrored fall,
//           0 at and past each span's span_lim.  The sample is computed here only when ks is the FIRST span of that greatest weight
//           (strict >, as patch_regions_kernel picks its window), so every written sample is written once, by one span's pass.
//   sample  si_wings of the staged row at file sample m: resample_sinc_kernel's arithmetic with the exact time in place of the
//           accumulated one.  The right wing's cap never binds (LONG_MAX): the row's zeros at and past win_lim end it.  Neighbouring
//           lanes read neighbouring LDS words (stride Q / P); the tables stay in L2 as they do for resample_sinc_kernel.  Nothing in it
//           depends on where the row or the chunk starts: same bits either way.
//   blend   g = gain * y; w == 1: g; else fma(w, g, (1 - w) * orig) -- patch_regions_kernel's roundings in its order; int16 files
//           read (float)v / 32768 and store through pc_pcm16's arithmetic.
// Every global access is one element wide, so orig / out / gen need only their element's alignment: callers pass views.  Plain stores, no
// atomics.  The C ABI validated on the host copy that every staged sample inside [0, win_lim) lies in its window's row; the staging
// loop still clamps to the row, so a device table that differs from the validated one gives wrong output, not a fault.
//
// INTER is the same workgroup for channel `channel` of an INTERLEAVED file (n_file sample times of ch channels):
// spans, chunks, fades and m are sample times of that channel, orig / out element m ch + channel (a 64-bit offset), and no other
// element of out is touched.  The table
// may name windows (rows of gen) and contexts (entries of gain) that none of its spans use: another channel's share of the pass.
template <typename T>
__device__ __forceinline__ void rk_patch_chunk(const T* __restrict__ orig, const SiRate& rt, const float* __restrict__ gen, int Lrow,
                                               const float* __restrict__ gain, int n_file, int ch, int channel, T* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rk_row[];
    const int q = blockIdx.x;
    const int c0 = rt.chunk[q] * RK_CHUNK, c1 = min(c0 + RK_CHUNK, n_file);
    const int k0 = rt.k0[q], k1 = rt.k1[q], fade = rt.fade;
    const long P = rt.r.P, Q = rt.r.Q;                                 // file sample i sits at 22.05 kHz position i Q / P
    const int H = rt.r.H;
    for (int ks = k0; ks < k1; ++ks) {                              // uniform
        const int s = rt.start[ks], l = rt.len[ks];
        const int ia = max(max(s - fade, 0), c0), ib = min(min(s + l + fade, rt.span_lim[ks]), c1);
        if (ia >= ib) continue;
        const int win = rt.span_win[ks];
        const int ws = rt.win_start[win], wl = rt.win_len[win], wlim = rt.win_lim[win];
        const int base = (int)((long)ia * Q / P) - H;
        const int cnt = min((int)((long)(ib - 1) * Q / P) + H + 1 - base, rt.row_cap);
        const float* __restrict__ grow = gen + (size_t)win * Lrow;
        __syncthreads();                                              // the previous span's readers are done with the row
        for (int p = threadIdx.x; p < cnt; p += 256) {
            const int j = base + p, o = j - ws;
            rk_row[p] = (j >= 0 && j < wlim && o >= 0 && o < wl) ? grow[o] : 0.f;
        }
        __syncthreads();
        const float g0 = gain ? gain[rt.win_ctx[win]] : 1.f;
        for (int m = ia + threadIdx.x; m < ib; m += 256) {
            float w = 0.f;
            int kw = -1;
            for (int k = k0; k < k1; ++k) {                           // uniform loop: patch_regions_kernel's walk
                if (m >= rt.span_lim[k]) continue;
                const int d = m - rt.start[k], lk = rt.len[k];
                float wk = 0.f;
                if (d < 0) { if (d >= -fade) wk = rt.ramp[d + fade]; }
                else if (d < lk) wk = 1.f;
                else if (d - lk < fade) wk = rt.ramp[fade - 1 - (d - lk)];
                if (wk > w) { w = wk; kw = k; }
            }
            if (kw != ks) continue;                                   // weight 0, or another span's pass writes it
            const float g = __fmul_rn(g0, si_wings(rk_row, (long)base, (long)m, LONG_MAX, rt.r));
            const size_t e = (size_t)m * ch + channel;
            rk_store(out + e, w == 1.f ? g : __fmaf_rn(w, g, __fmul_rn(1.f - w, rk_load(orig + e))));
        }
    }
}

template <typename T, bool INTER>
__global__ __launch_bounds__(256) void patch_rate_kernel(const T* __restrict__ orig, SiRate rt, const float* __restrict__ gen, int Lrow,
                                                         const float* __restrict__ gain, int n_file, int ch, int channel, T* __restrict__ out) {
    rk_patch_chunk(orig, rt, gen, Lrow, gain, n_file, INTER ? ch : 1, INTER ? channel : 0, out);
}

// ch = 0: the mono kernel under "patch_rate"; else the interleaved one under "patch_rate_ch".  The caller (si_patch_rate[_ch]) checked
// every argument, row_cap * 4 <= 64 KB, 1 <= ch <= SI_MAX_CHANNELS and 0 <= channel < ch among them.
int si_launch_patch_rate(si_ctx* ctx, const void* orig, int fmt, int n_file, int ch, int channel, const SiRate& rt, int num_chunks,
                         const float* gen, int Lrow, const float* gain, void* out, hipStream_t st) {
    if (num_chunks <= 0) return SI_OK;
    const size_t lds = (size_t)rt.row_cap * sizeof(float);
    const double esz = si_sample_bytes(fmt);
    si_prof_begin(ctx, ch > 0 ? "patch_rate_ch" : "patch_rate", (double)num_chunks * RK_CHUNK * 8.0 * rt.r.H,
                  (double)num_chunks * (RK_CHUNK * 2.0 * esz + 4.0 * rt.row_cap), st);
    si_with_sample(fmt, [&](auto tag) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(tag)>>;
        si_with_flag(ch > 0, [&](auto inter) {
            patch_rate_kernel<T, decltype(inter)::value><<<dim3(num_chunks), 256, lds, st>>>(static_cast<const T*>(orig), rt, gen, Lrow, gain, n_file, ch,
                                                                                             channel, static_cast<T*>(out));
        });
    });
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}
