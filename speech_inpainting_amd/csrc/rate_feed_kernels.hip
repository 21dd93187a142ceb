// rate_feed_kernels.hip -- the model's 22.05 kHz context clips cut straight out of a file at its own rate, gfx950.
//   cut_rate_kernel<float | int16_t | SiS24>   per tile of 512 consecutive outputs of one clip: the file samples the tile's interpolation reads
//                                      staged in LDS as fp32, then per output the two wings of the band-limited interpolation at the
//                                      exact rational time j Q / P
//   cut_rate_ch_kernel<float | int16_t>  the same tile read from one channel of an INTERLEAVED file: one shared body
//   cut_rate_valid_kernel, cut_rate_valid_ch_kernel, cut_pair_valid_kernel, cut_pair_valid_ch_kernel
//                                      the same bodies with an INVALID file sample (NaN, +-inf, |x| > ceiling) staged as +0.0
//   cut_pair_kernel, cut_pair_ch_kernel  per 20 ms frame of one clip, its 22.05 kHz AND its 16 kHz samples from one staged range (DESIGN.md
//                                      4.26; further down, with its own description)
// It stands where `resample(file, sr, 22050)` over the whole recording + si_cut_clips would: that pass costs every 22.05 kHz sample of
// the recording a 2 H-tap float64 sum, an fp32 copy of an int16 file, a 22.05 kHz copy of the recording and a float64 time table of its
// length; this one computes the samples of the context clips and creates nothing of the recording's length.
#include "common.h"

__device__ __forceinline__ float rf_load(const float* p) { return *p; }
__device__ __forceinline__ float rf_load(const int16_t* p) { return (float)*p * (1.0f / 32768.0f); }     // exact: 16 bits x 2^-15
__device__ __forceinline__ float rf_load(const SiS24* p) { return (float)p->value() * (1.0f / 8388608.0f); }  // exact: 24 bits x 2^-23

// What the staging statement of both tile bodies reads for one existing file sample.  CLEAN = false: rf_load, the text it always was.
// CLEAN = true (the _valid entry points): a sample that is si_invalid(., ceiling) -- judged in the file's own units,
// before the conversion -- enters as +0.0; every other sample as rf_load gives it.  Nothing behind the staging loop knows the policy.
template <bool CLEAN, typename T>
__device__ __forceinline__ float rf_feed(const T* p, float ceiling) {
    if constexpr (CLEAN) {
        const T v = *p;
        return si_invalid(v, ceiling) ? 0.f : rf_load(&v);
    } else {
        return rf_load(p);
    }
}

// grid (ceil(L / 512), C), 256 threads, fd.cap floats of dynamic LDS.  Workgroup (tile, c) owns outputs [tile 512, min(tile 512 + 512, L))
// of clip c = 22.05 kHz samples j0 + [0, cnt) of the recording, j0 = start[c] + tile 512 (workgroup-uniform: scalar loads).
//   stage   file samples [n0 - H, n1 + H], n0 = floor(j0 Q / P), n1 = floor((j0 + cnt - 1) Q / P): lane t loads element t, t + 256, ...
//           (one element wide: coalesced whatever the file's alignment -- callers pass views), int16 converted on the way in, zero before
//           file sample 0 and at / past n_file.  n1 - n0 <= floor(511 Q / P) + 1, so the range holds at most
//           floor(511 Q / P) + 2 + 2 H = cap samples: 65 taps per wing when up-sampling, 140 at 48 kHz, 565 at 192 kHz (5 582 floats).
//   sample  lane t owns outputs t and t + 256.  n, r = divmod(j Q, P) in int64; frac = scale (r / P); left wing off, eta =
//           split(frac num_table), taps k < min(n + 1, (nwin - off) / step) on x[n - k]; right wing the same from scale - frac, taps
//           k < min(n_file - n - 1, (nwin - off') / step) on x[n + 1 + k]; weights fma(eta, dwin, win), sum by fma in float64, left
//           ascending then right ascending, rounded once to fp32: resample_sinc_kernel's arithmetic at the exact time.  Neighbouring
//           lanes read neighbouring LDS words (stride Q / P); the tables stay in L2 as they do for resample_sinc_kernel.  Nothing in
//           it depends on where the clip or the tile starts: a sample has the same bits in whichever clip it is cut.
// Plain stores, no atomics; each output is written once.  The C ABI validated the host copy of `start`; an output whose j lies outside
// [0, N22) -- a device table that differs from the validated one -- is written as zero, and the staging loop reads the file only inside
// [0, n_file): wrong output, not a fault.
//
// cut_rate_ch_kernel is the same workgroup reading channel `channel` of an INTERLEAVED file (n_file sample times of ch
// channels, element i ch + channel): one body, rf_cut_tile, serves both, the mono kernel with ch = 1, channel = 0 folded in.  The staging
// loop clamps on the sample TIME before it forms the 64-bit element offset, so a time outside [0, n_file) is zero, never the neighbouring
// channel's element; everything after the staging is the mono arithmetic on the staged fp32 row.
template <typename T, bool CLEAN>
__device__ __forceinline__ void rf_cut_tile(const T* __restrict__ x, int n_file, int ch, int channel, const int32_t* __restrict__ start, int L,
                                            const SiFeed& fd, float ceiling, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rf_row[];
    const int c = blockIdx.y, o0 = blockIdx.x * RF_TILE;
    const int cnt = min(RF_TILE, L - o0);
    const long j0 = (long)start[c] + o0;
    const long P = fd.P, Q = fd.Q;
    const int H = fd.H, nwin = fd.nwin, step = fd.step;
    const double scale = fd.scale, ntab = (double)fd.num_table;
    const bool live = j0 >= 0 && j0 + cnt <= (long)fd.N22;              // uniform
    const long base = live ? j0 * Q / P - H : 0;
    const int span = live ? min((int)((j0 + cnt - 1) * Q / P + H + 1 - base), fd.cap) : 0;
    for (int p = threadIdx.x; p < span; p += 256) {
        const long i = base + p;
        rf_row[p] = (i >= 0 && i < (long)n_file) ? rf_feed<CLEAN>(x + ((size_t)i * ch + channel), ceiling) : 0.f;
    }
    __syncthreads();
    float* orow = out + (size_t)c * L + o0;
    for (int m = threadIdx.x; m < cnt; m += 256) {
        if (!live) { orow[m] = 0.f; continue; }
        const long t = (j0 + m) * Q;
        const long nl = t / P;
        const int n = (int)nl;
        const double frac = scale * ((double)(t - nl * P) / (double)P);
        double acc = 0.0;
        {
            const double idx = frac * ntab;
            const int off = (int)idx;
            const double eta = idx - (double)off;
            const int taps = min(n + 1, (nwin - off) / step);
            const float* xs = rf_row + (nl - base);
            for (int k = 0; k < taps; ++k) {
                const int i = off + k * step;
                acc = fma(fma(eta, fd.dwin[i], fd.win[i]), (double)xs[-k], acc);
            }
        }
        {
            const double idx = (scale - frac) * ntab;
            const int off = (int)idx;
            const double eta = idx - (double)off;
            const int taps = min(n_file - n - 1, (nwin - off) / step);
            const float* xs = rf_row + (nl + 1 - base);
            for (int k = 0; k < taps; ++k) {
                const int i = off + k * step;
                acc = fma(fma(eta, fd.dwin[i], fd.win[i]), (double)xs[k], acc);
            }
        }
        orow[m] = (float)acc;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void cut_rate_kernel(const T* __restrict__ x, int n_file, const int32_t* __restrict__ start, int L, SiFeed fd,
                                                       float* __restrict__ out) {
    rf_cut_tile<T, false>(x, n_file, 1, 0, start, L, fd, 0.f, out);
}

template <typename T>
__global__ __launch_bounds__(256) void cut_rate_ch_kernel(const T* __restrict__ x, int n_file, int ch, int channel, const int32_t* __restrict__ start,
                                                          int L, SiFeed fd, float* __restrict__ out) {
    rf_cut_tile<T, false>(x, n_file, ch, channel, start, L, fd, 0.f, out);
}

// The same two kernels with an invalid file sample staged as +0.0: rf_cut_tile<T, true>.
template <typename T>
__global__ __launch_bounds__(256) void cut_rate_valid_kernel(const T* __restrict__ x, int n_file, const int32_t* __restrict__ start, int L, SiFeed fd,
                                                             float ceiling, float* __restrict__ out) {
    rf_cut_tile<T, true>(x, n_file, 1, 0, start, L, fd, ceiling, out);
}

template <typename T>
__global__ __launch_bounds__(256) void cut_rate_valid_ch_kernel(const T* __restrict__ x, int n_file, int ch, int channel,
                                                                const int32_t* __restrict__ start, int L, SiFeed fd, float ceiling,
                                                                float* __restrict__ out) {
    rf_cut_tile<T, true>(x, n_file, ch, channel, start, L, fd, ceiling, out);
}

// ---- both clip sets of a pass from one staged tile
//   cut_pair_kernel<float | int16_t>     per RF_PAIR_FRAMES consecutive 20 ms frames of one clip: the file samples that BOTH rates read for
//                                        them staged once in LDS as fp32, then the frames' 441 F outputs at 22.05 kHz and 320 F at 16 kHz
//   cut_pair_ch_kernel<float | int16_t>  the same tile read from one channel of an INTERLEAVED file: one shared body, rf_pair_tile
// grid (max(ceil(L22 / 441 F), ceil(L16 / 320 F)), C), 256 threads, pr.cap floats of dynamic LDS.  Workgroup (tile, c) owns frames
// f0 + [0, F), f0 = frame[c] + tile F (workgroup-uniform): 22.05 kHz samples 441 f0 + [0, cnt22) and 16 kHz samples 320 f0 + [0, cnt16).
//   stage   both rows start at the SAME file position f0 sr / 50 (441 f0 Q22 / P22 = 320 f0 Q16 / P16), so n0 = floor of it is shared;
//           n1 = the larger last integer part of the two; file samples [n0 - H, n1 + H], H = max(H22, H16), by cut_rate's staging loop
//           (lane t on element t, one element wide, int16 converted on the way in, zero outside [0, n_file), the sample TIME clamped
//           before the 64-bit element offset of an interleaved file is formed).  Every output's time lies in [f0, f0 + F) / 50 s, so
//           n1 - n0 <= ceil(F sr / 50) and the range holds at most ceil(F sr / 50) + 1 + 2 H <= cap samples.
//   sample  one index space over the tile's cnt22 + cnt16 outputs, lane t on t, t + 256, ...: rf_wings is rf_cut_tile's per-output
//           arithmetic, statement for statement, on the tables of the output's rate -- a 22.05 kHz output has si_cut_rate's bits.  A
//           16 kHz output with j >= N16 (at or past the file's end: at most the one the L16 rule allows) is +0.0; at sr = 16000 the
//           output is the staged sample itself, n = j, no table read.  Neighbouring lanes read LDS words Q / P apart, as in cut_rate:
//           an even integer stride (32 kHz: 2, 192 kHz: 12) costs ds_read_b32 a 2- or 4-way bank conflict, under two float64 fma and
//           two float64 table loads per tap.
// Plain stores, no atomics; each output is written once.  A device frame table that differs from the validated host copy: a tile whose
// outputs leave [0, N22) / [0, lim16) is written as zero, and the staging loop reads the file only inside [0, n_file).
__device__ __forceinline__ float rf_wings(const float* __restrict__ row, long base, long j, int n_file, const SiPairRate& r) {
    const long P = r.P, Q = r.Q;
    const int nwin = r.nwin, step = r.step;
    const double scale = r.scale, ntab = (double)r.num_table;
    const long t = j * Q;
    const long nl = t / P;
    const int n = (int)nl;
    const double frac = scale * ((double)(t - nl * P) / (double)P);
    double acc = 0.0;
    {
        const double idx = frac * ntab;
        const int off = (int)idx;
        const double eta = idx - (double)off;
        const int taps = min(n + 1, (nwin - off) / step);
        const float* xs = row + (nl - base);
        for (int k = 0; k < taps; ++k) {
            const int i = off + k * step;
            acc = fma(fma(eta, r.dwin[i], r.win[i]), (double)xs[-k], acc);
        }
    }
    {
        const double idx = (scale - frac) * ntab;
        const int off = (int)idx;
        const double eta = idx - (double)off;
        const int taps = min(n_file - n - 1, (nwin - off) / step);
        const float* xs = row + (nl + 1 - base);
        for (int k = 0; k < taps; ++k) {
            const int i = off + k * step;
            acc = fma(fma(eta, r.dwin[i], r.win[i]), (double)xs[k], acc);
        }
    }
    return (float)acc;
}

template <typename T, bool CLEAN>
__device__ __forceinline__ void rf_pair_tile(const T* __restrict__ x, int n_file, int ch, int channel, const int32_t* __restrict__ frame, int L22,
                                             int L16, const SiPair& pr, float ceiling, float* __restrict__ out22, float* __restrict__ out16) {
    extern __shared__ __attribute__((aligned(16))) float rf_pair_row[];
    constexpr int T22 = 441 * RF_PAIR_FRAMES, T16 = 320 * RF_PAIR_FRAMES;
    const int c = blockIdx.y, o22 = blockIdx.x * T22, o16 = blockIdx.x * T16;
    const int cnt22 = max(0, min(T22, L22 - o22)), cnt16 = max(0, min(T16, L16 - o16));
    const long fc = frame[c];
    const long f0 = fc + (long)blockIdx.x * RF_PAIR_FRAMES;
    const long j22 = 441 * f0, j16 = 320 * f0;
    const bool live22 = fc >= 0 && cnt22 > 0 && j22 + cnt22 <= (long)pr.N22;        // uniform
    const bool live16 = fc >= 0 && cnt16 > 0 && j16 + cnt16 <= (long)pr.lim16;      // uniform
    const int H = max(pr.r22.H, pr.r16.H);
    const long n0 = j22 * pr.r22.Q / pr.r22.P;                                      // = floor(j16 Q16 / P16): the frame's own file position
    long n1 = n0;
    if (live22) n1 = max(n1, (j22 + cnt22 - 1) * pr.r22.Q / pr.r22.P);
    if (live16) n1 = max(n1, (j16 + cnt16 - 1) * pr.r16.Q / pr.r16.P);
    const long base = (live22 || live16) ? n0 - H : 0;
    const int span = (live22 || live16) ? (int)min(n1 + H + 1 - base, (long)pr.cap) : 0;
    for (int p = threadIdx.x; p < span; p += 256) {
        const long i = base + p;
        rf_pair_row[p] = (i >= 0 && i < (long)n_file) ? rf_feed<CLEAN>(x + ((size_t)i * ch + channel), ceiling) : 0.f;
    }
    __syncthreads();
    float* row22 = out22 + (size_t)c * L22 + o22;
    float* row16 = out16 + (size_t)c * L16 + o16;
    for (int m = threadIdx.x; m < cnt22 + cnt16; m += 256) {
        if (m < cnt22) {
            row22[m] = live22 ? rf_wings(rf_pair_row, base, j22 + m, n_file, pr.r22) : 0.f;
            continue;
        }
        const int m16 = m - cnt22;
        const long j = j16 + m16;
        float y = 0.f;
        if (live16 && j < (long)pr.N16) y = pr.direct16 ? rf_pair_row[j - base] : rf_wings(rf_pair_row, base, j, n_file, pr.r16);
        row16[m16] = y;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void cut_pair_kernel(const T* __restrict__ x, int n_file, const int32_t* __restrict__ frame, int L22, int L16,
                                                       SiPair pr, float* __restrict__ out22, float* __restrict__ out16) {
    rf_pair_tile<T, false>(x, n_file, 1, 0, frame, L22, L16, pr, 0.f, out22, out16);
}

template <typename T>
__global__ __launch_bounds__(256) void cut_pair_ch_kernel(const T* __restrict__ x, int n_file, int ch, int channel, const int32_t* __restrict__ frame,
                                                          int L22, int L16, SiPair pr, float* __restrict__ out22, float* __restrict__ out16) {
    rf_pair_tile<T, false>(x, n_file, ch, channel, frame, L22, L16, pr, 0.f, out22, out16);
}

// The same two kernels with an invalid file sample staged as +0.0: rf_pair_tile<T, true>.  At sr = 16000 the unfiltered
// 16 kHz row is the STAGED sample, so it is +0.0 there too.
template <typename T>
__global__ __launch_bounds__(256) void cut_pair_valid_kernel(const T* __restrict__ x, int n_file, const int32_t* __restrict__ frame, int L22, int L16,
                                                             SiPair pr, float ceiling, float* __restrict__ out22, float* __restrict__ out16) {
    rf_pair_tile<T, true>(x, n_file, 1, 0, frame, L22, L16, pr, ceiling, out22, out16);
}

template <typename T>
__global__ __launch_bounds__(256) void cut_pair_valid_ch_kernel(const T* __restrict__ x, int n_file, int ch, int channel,
                                                                const int32_t* __restrict__ frame, int L22, int L16, SiPair pr, float ceiling,
                                                                float* __restrict__ out22, float* __restrict__ out16) {
    rf_pair_tile<T, true>(x, n_file, ch, channel, frame, L22, L16, pr, ceiling, out22, out16);
}

// The caller (si_cut_pair[_ch]) checked every argument, pr.cap * 4 <= 64 KB and C <= 65535 among them.  ch = 0: the mono kernel.  The
// launches are profiled under cut_rate's names: the same family, and like it they hold no scratch of the context's.
int si_launch_cut_pair(si_ctx* ctx, const void* x, int fmt, int n_file, int ch, int channel, const int32_t* frame, int C, int L22, int L16,
                       const SiPair& pr, float* out22, float* out16, hipStream_t st) {
    if (C <= 0 || L22 <= 0 || L16 <= 0) return SI_OK;
    constexpr int T22 = 441 * RF_PAIR_FRAMES, T16 = 320 * RF_PAIR_FRAMES;
    const size_t lds = (size_t)pr.cap * sizeof(float);
    const dim3 grid(std::max((L22 + T22 - 1) / T22, (L16 + T16 - 1) / T16), C);
    const double o22 = (double)C * L22, o16 = (double)C * L16;
    const double flops = o22 * 8.0 * pr.r22.H + o16 * 8.0 * pr.r16.H;
    const double bytes = (o22 + o16) * 4.0 + (double)grid.x * C * pr.cap * si_sample_bytes(fmt);
    if (ch > 0) {
        si_prof_begin(ctx, "cut_rate_ch", flops, bytes, st);
        si_with_sample(fmt, [&](auto tag) {
            using T = std::remove_const_t<std::remove_pointer_t<decltype(tag)>>;
            cut_pair_ch_kernel<T><<<grid, 256, lds, st>>>(static_cast<const T*>(x), n_file, ch, channel, frame, L22, L16, pr, out22, out16);
        });
    } else {
        si_prof_begin(ctx, "cut_rate", flops, bytes, st);
        si_with_sample(fmt, [&](auto tag) {
            using T = std::remove_const_t<std::remove_pointer_t<decltype(tag)>>;
            cut_pair_kernel<T><<<grid, 256, lds, st>>>(static_cast<const T*>(x), n_file, frame, L22, L16, pr, out22, out16);
        });
    }
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}

// The caller (si_cut_rate) checked every argument, fd.cap * 4 <= 64 KB and C <= 65535 among them.
int si_launch_cut_rate(si_ctx* ctx, const void* x, int fmt, int n_file, const int32_t* start, int C, int L, const SiFeed& fd, float* out,
                       hipStream_t st) {
    if (C <= 0 || L <= 0) return SI_OK;
    const size_t lds = (size_t)fd.cap * sizeof(float);
    const dim3 grid((L + RF_TILE - 1) / RF_TILE, C);
    const double outs = (double)C * L;
    si_prof_begin(ctx, "cut_rate", outs * 8.0 * fd.H, outs * 4.0 + (double)grid.x * C * fd.cap * si_sample_bytes(fmt), st);
    si_with_sample(fmt, [&](auto tag) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(tag)>>;
        cut_rate_kernel<T><<<grid, 256, lds, st>>>(static_cast<const T*>(x), n_file, start, L, fd, out);
    });
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}

// The caller (si_cut_rate_ch) checked every argument, 1 <= ch <= SI_MAX_CHANNELS and 0 <= channel < ch among them.
int si_launch_cut_rate_ch(si_ctx* ctx, const void* x, int fmt, int n_file, int ch, int channel, const int32_t* start, int C, int L,
                          const SiFeed& fd, float* out, hipStream_t st) {
    if (C <= 0 || L <= 0) return SI_OK;
    const size_t lds = (size_t)fd.cap * sizeof(float);
    const dim3 grid((L + RF_TILE - 1) / RF_TILE, C);
    const double outs = (double)C * L;
    si_prof_begin(ctx, "cut_rate_ch", outs * 8.0 * fd.H, outs * 4.0 + (double)grid.x * C * fd.cap * si_sample_bytes(fmt), st);
    si_with_sample(fmt, [&](auto tag) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(tag)>>;
        cut_rate_ch_kernel<T><<<grid, 256, lds, st>>>(static_cast<const T*>(x), n_file, ch, channel, start, L, fd, out);
    });
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}

// ---- the feeds that stage an invalid file sample as +0.0
// si_launch_cut_rate[_ch] and si_launch_cut_pair with the CLEAN instantiations: the same grids, the same LDS, the same profile names
// (ch = 0: the mono kernel under "cut_rate"; else "cut_rate_ch").  The callers (si_cut_rate_valid, si_cut_pair_valid) checked every
// argument, the ceiling among them.
int si_launch_cut_rate_valid(si_ctx* ctx, const void* x, int fmt, int n_file, int ch, int channel, const int32_t* start, int C, int L,
                             const SiFeed& fd, float ceiling, float* out, hipStream_t st) {
    if (C <= 0 || L <= 0) return SI_OK;
    const size_t lds = (size_t)fd.cap * sizeof(float);
    const dim3 grid((L + RF_TILE - 1) / RF_TILE, C);
    const double outs = (double)C * L;
    si_prof_begin(ctx, ch > 0 ? "cut_rate_ch" : "cut_rate", outs * 8.0 * fd.H, outs * 4.0 + (double)grid.x * C * fd.cap * si_sample_bytes(fmt), st);
    si_with_sample(fmt, [&](auto tag) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(tag)>>;
        if (ch > 0) cut_rate_valid_ch_kernel<T><<<grid, 256, lds, st>>>(static_cast<const T*>(x), n_file, ch, channel, start, L, fd, ceiling, out);
        else cut_rate_valid_kernel<T><<<grid, 256, lds, st>>>(static_cast<const T*>(x), n_file, start, L, fd, ceiling, out);
    });
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}

int si_launch_cut_pair_valid(si_ctx* ctx, const void* x, int fmt, int n_file, int ch, int channel, const int32_t* frame, int C, int L22,
                             int L16, const SiPair& pr, float ceiling, float* out22, float* out16, hipStream_t st) {
    if (C <= 0 || L22 <= 0 || L16 <= 0) return SI_OK;
    constexpr int T22 = 441 * RF_PAIR_FRAMES, T16 = 320 * RF_PAIR_FRAMES;
    const size_t lds = (size_t)pr.cap * sizeof(float);
    const dim3 grid(std::max((L22 + T22 - 1) / T22, (L16 + T16 - 1) / T16), C);
    const double o22 = (double)C * L22, o16 = (double)C * L16;
    const double flops = o22 * 8.0 * pr.r22.H + o16 * 8.0 * pr.r16.H;
    const double bytes = (o22 + o16) * 4.0 + (double)grid.x * C * pr.cap * si_sample_bytes(fmt);
    si_prof_begin(ctx, ch > 0 ? "cut_rate_ch" : "cut_rate", flops, bytes, st);
    si_with_sample(fmt, [&](auto tag) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(tag)>>;
        if (ch > 0)
            cut_pair_valid_ch_kernel<T><<<grid, 256, lds, st>>>(static_cast<const T*>(x), n_file, ch, channel, frame, L22, L16, pr, ceiling, out22, out16);
        else
            cut_pair_valid_kernel<T><<<grid, 256, lds, st>>>(static_cast<const T*>(x), n_file, frame, L22, L16, pr, ceiling, out22, out16);
    });
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}
