// patch_kernels.hip -- patch mode, gfx950: the generated audio of the gaps spliced into the caller's own 22.05 kHz
// samples.  Two HBM-side kernels around the ragged generator pass:
//   gather_windows_kernel   stretched-mel windows (clip, w0, w1) of ext (B, D, Tout) -> the generator's ragged input (W, D, Wmax)
//   patch_compose_kernel    out = orig outside the blend regions, (1 - w) orig + w gain gen inside them (+ the int16 conversion)
// The time map between the generator's samples and the input's is the identity (vocoder_kernels.hip, extend_mel: stretched frame t is
// centred at input sample (t + 0.5) * 256 and the generator emits 256 samples per stretched frame), so sample m of a window row that
// starts at stretched frame w0 is input sample w0 * hop + m: no resampling, no drift.
// Recordings longer than one clip add the two ends of the route that serves them as context clips:
//   cut_clips_kernel        rows src[start[c] : start[c] + L] of the 1-D recording -> the context clips (C, L), either sample rate
//   patch_regions_kernel    the blended samples of many contexts' gaps written straight into the one long output, chunk by touched chunk
#include "common.h"

// ------------------------------------------------------------------------------------------------ window gather
// grid (ceil(D / 4), W), 256 threads: one wave copies one (window, channel) row of w1 - w0 floats and zero-fills it up to Wmax.
// w0 is arbitrary, so the source row is generally not 16-byte aligned: alignment is decided PER ROW and per side -- a destination row
// that is aligned gets 16-byte stores, fed by 16-byte loads when the source row is aligned too and by scalar loads otherwise; a
// destination row that is not (Wmax not a multiple of 4) is copied by scalar accesses.
__global__ __launch_bounds__(256) void gather_windows_kernel(const float* __restrict__ ext, const int32_t* __restrict__ win, int W, int D, int Tout,
                                                             int Wmax, float* __restrict__ out) {
    const int w = blockIdx.y, d = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (d >= D) return;
    const int clip = win[w], w0 = win[W + w], len = win[2 * W + w] - w0;
    const float* src = ext + ((size_t)clip * D + d) * Tout + w0;
    float* dst = out + ((size_t)w * D + d) * Wmax;
    const bool dvec = (reinterpret_cast<size_t>(dst) & 15) == 0, svec = (reinterpret_cast<size_t>(src) & 15) == 0;
    const int n4 = dvec ? (Wmax & ~3) : 0;
    for (int i = lane * 4; i < n4; i += 64 * 4) {
        float4 v;
        if (svec && i + 4 <= len) {
            v = *reinterpret_cast<const float4*>(src + i);
        } else {
            v.x = i < len ? src[i] : 0.f;
            v.y = i + 1 < len ? src[i + 1] : 0.f;
            v.z = i + 2 < len ? src[i + 2] : 0.f;
            v.w = i + 3 < len ? src[i + 3] : 0.f;
        }
        *reinterpret_cast<float4*>(dst + i) = v;
    }
    for (int i = n4 + lane; i < Wmax; i += 64) dst[i] = i < len ? src[i] : 0.f;
}

int si_launch_gather_windows(si_ctx* ctx, const float* ext, const int32_t* win, int W, int D, int Tout, int Wmax, float* out, hipStream_t st) {
    if (W <= 0) return SI_OK;
    si_prof_begin(ctx, "gather_windows", 0.0, 8.0 * W * D * Wmax, st);
    gather_windows_kernel<<<dim3((D + 3) / 4, W), 256, 0, st>>>(ext, win, W, D, Tout, Wmax, out);
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}

// ------------------------------------------------------------------------------------------------ compose
// pcm16_kernel's arithmetic (frontend_kernels.hip; I_ea/predict.py:204-206): `* 32768`, truncated toward zero, 32768.0 -> 32767, NaN -> 0
__device__ __forceinline__ short pc_pcm16(float v) {
    const float p = v * 32768.0f;
    return (short)(int)fminf(fmaxf(truncf(p == p ? p : 0.f), -32768.f), 32767.f);
}

constexpr int PC_CHUNK = 2048;      // samples per workgroup: 256 lanes x two 16-byte loads; 88 200 samples x 32 clips = 1408 workgroups

// grid (ceil(N22 / PC_CHUNK), B), 256 threads.  One workgroup owns samples [c0, c1) of clip b.  It walks the clip's spans ONCE (b is
// workgroup-uniform: the table arrives through scalar loads) to learn whether a blend region [max(s - fade, 0), min(e + fade, lim))
// meets its chunk.  Nearly every chunk meets none and is a straight copy, 16 bytes per lane where the row is aligned, fused with the
// int16 conversion; the few that do run the per-sample path:
//     w(m) = max over the clip's spans of { ramp[m - (s - fade)] on the rise, 1 in [s, e), ramp[e + fade - 1 - m] on the fall }, 0 for m >= lim
//     w == 0: the original's bits (the copy branch: -0.0 and NaN payloads survive, which `x + 0` would not guarantee)
//     w == 1: exactly the fp32 product gain * gen
//     else  : fma(w, gain * gen, (1 - w) * orig) -- four roundings: 1 - w, its product, gain * gen, the fma
// gen holds one row of Lrow samples per window; a span's samples come from ITS window (span_win), row sample m - win_start.  The C ABI
// checked on the host copy that every region lies inside its window's row, so no index leaves gen.  Plain vector stores throughout.
__global__ __launch_bounds__(256) void patch_compose_kernel(const float* __restrict__ orig, SiSpans sp, SiPatch pt, const float* __restrict__ gen, int Lrow,
                                                            const float* __restrict__ gain, int N22, float* __restrict__ out, int16_t* __restrict__ pcm) {
    const int b = blockIdx.y;
    const int c0 = blockIdx.x * PC_CHUNK, c1 = min(c0 + PC_CHUNK, N22);
    const int k0 = sp.off[b], k1 = sp.off[b + 1];
    const int lim = pt.lim[b], fade = pt.fade;
    bool blend = false;
    for (int k = k0; k < k1; ++k) {
        const int s = sp.start[k], l = sp.len[k];
        if (l <= 0 || s >= lim) continue;
        const int e = min(s + l, lim);
        blend |= max(s - fade, 0) < c1 && min(e + fade, lim) > c0;
    }
    const float* x = orig + (size_t)b * N22;
    float* o = out ? out + (size_t)b * N22 : nullptr;
    int16_t* q = pcm ? pcm + (size_t)b * N22 : nullptr;
    if (!blend) {
        // c0 is a multiple of PC_CHUNK, so the row's alignment is the chunk's (N22 not a multiple of 4: three rows of four are scalar)
        const bool vec = (reinterpret_cast<size_t>(x) & 15) == 0 && (reinterpret_cast<size_t>(o) & 15) == 0 && (reinterpret_cast<size_t>(q) & 7) == 0;
#pragma unroll
        for (int r = 0; r < PC_CHUNK / 1024; ++r) {
            const int i = c0 + r * 1024 + threadIdx.x * 4;
            if (vec && i + 4 <= c1) {
                const float4 v = *reinterpret_cast<const float4*>(x + i);
                if (o) *reinterpret_cast<float4*>(o + i) = v;
                if (q) *reinterpret_cast<short4*>(q + i) = make_short4(pc_pcm16(v.x), pc_pcm16(v.y), pc_pcm16(v.z), pc_pcm16(v.w));
            } else {
                for (int j = i; j < c1 && j < i + 4; ++j) {
                    const float v = x[j];
                    if (o) o[j] = v;
                    if (q) q[j] = pc_pcm16(v);
                }
            }
        }
        return;
    }
    const float g0 = gain ? gain[b] : 1.f;
    for (int m = c0 + threadIdx.x; m < c1; m += 256) {
        float w = 0.f;
        int win = 0;
        if (m < lim) {
            for (int k = k0; k < k1; ++k) {                          // uniform loop: s, l, span_win come through scalar loads
                const int s = sp.start[k], l = sp.len[k];
                if (l <= 0 || s >= lim) continue;
                const int d = m - s;
                float wk = 0.f;
                if (d < 0) { if (d >= -fade) wk = pt.ramp[d + fade]; }
                else if (d < l) wk = 1.f;
                else if (d - l < fade) wk = pt.ramp[fade - 1 - (d - l)];
                if (wk > w) { w = wk; win = pt.span_win[k]; }
            }
        }
        float v = x[m];
        if (w != 0.f) {
            const float g = __fmul_rn(g0, gen[(size_t)win * Lrow + (m - pt.win_start[win])]);
            v = w == 1.f ? g : __fmaf_rn(w, g, __fmul_rn(1.f - w, v));
        }
        if (o) o[m] = v;
        if (q) q[m] = pc_pcm16(v);
    }
}

int si_launch_patch_compose(si_ctx* ctx, const float* orig, const SiSpans& sp, const SiPatch& pt, const float* gen, int Lrow, const float* gain,
                            int B, int N22, float* out, int16_t* pcm, hipStream_t st) {
    if (B <= 0 || N22 <= 0) return SI_OK;
    si_prof_begin(ctx, "patch_compose", 0.0, (double)B * N22 * (4.0 + (out ? 4.0 : 0.0) + (pcm ? 2.0 : 0.0)), st);
    patch_compose_kernel<<<dim3((N22 + PC_CHUNK - 1) / PC_CHUNK, B), 256, 0, st>>>(orig, sp, pt, gen, Lrow, gain, N22, out, pcm);
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}

// ------------------------------------------------------------------------------------------------ long recordings
// grid (ceil(L / PC_CHUNK), C), 256 threads: one workgroup copies samples [x0, x1) of context clip c from src + start[c].  start is
// 441 f or 320 f, so the source row is generally off the 16-byte grid, and the destination row is when L % 4 != 0: alignment is decided
// PER ROW and per side as in gather_windows_kernel (x0 is a multiple of PC_CHUNK, so a chunk has its row's alignment) -- 16-byte stores
// into an aligned destination, fed by 16-byte loads when the source row is aligned too and by scalar loads otherwise; scalar accesses
// into a destination that is not.  The C ABI checked 0 <= start and start + L <= n_src on the host copy.
// CLEAN = true (si_cut_clips_valid) copies a sample that is si_invalid(., ceiling) as +0.0; CLEAN = false is the copy as
// it always was, bits unchanged.
template <bool CLEAN>
__device__ __forceinline__ float pc_feed(float v, float ceiling) {
    if constexpr (CLEAN) return si_invalid(v, ceiling) ? 0.f : v;
    else return v;
}

template <bool CLEAN>
__device__ __forceinline__ void pc_cut_clips(const float* __restrict__ src, const int32_t* __restrict__ start, int L, float ceiling,
                                             float* __restrict__ out) {
    const int c = blockIdx.y;
    const int x0 = blockIdx.x * PC_CHUNK, x1 = min(x0 + PC_CHUNK, L);
    const float* s = src + (size_t)start[c];
    float* d = out + (size_t)c * L;
    const bool dvec = (reinterpret_cast<size_t>(d) & 15) == 0, svec = (reinterpret_cast<size_t>(s) & 15) == 0;
#pragma unroll
    for (int r = 0; r < PC_CHUNK / 1024; ++r) {
        const int i = x0 + r * 1024 + threadIdx.x * 4;
        if (dvec && i + 4 <= x1) {
            float4 v;
            if (svec) {
                v = *reinterpret_cast<const float4*>(s + i);
                v.x = pc_feed<CLEAN>(v.x, ceiling);
                v.y = pc_feed<CLEAN>(v.y, ceiling);
                v.z = pc_feed<CLEAN>(v.z, ceiling);
                v.w = pc_feed<CLEAN>(v.w, ceiling);
            } else {
                v.x = pc_feed<CLEAN>(s[i], ceiling);
                v.y = pc_feed<CLEAN>(s[i + 1], ceiling);
                v.z = pc_feed<CLEAN>(s[i + 2], ceiling);
                v.w = pc_feed<CLEAN>(s[i + 3], ceiling);
            }
            *reinterpret_cast<float4*>(d + i) = v;
        } else {
            for (int j = i; j < x1 && j < i + 4; ++j) d[j] = pc_feed<CLEAN>(s[j], ceiling);
        }
    }
}

template <bool CLEAN>
__global__ __launch_bounds__(256) void cut_clips_kernel(const float* __restrict__ src, const int32_t* __restrict__ start, int L, float ceiling,
                                                        float* __restrict__ out) {
    pc_cut_clips<CLEAN>(src, start, L, ceiling, out);
}

// ceiling = nullptr: the copy as it always was; else (si_cut_clips_valid, which checked it) the CLEAN one: the same grid and profile name.
int si_launch_cut_clips(si_ctx* ctx, const float* src, const int32_t* start, int C, int L, const float* ceiling, float* out, hipStream_t st) {
    if (C <= 0 || L <= 0) return SI_OK;
    si_prof_begin(ctx, "cut_clips", 0.0, 8.0 * C * L, st);
    si_with_flag(ceiling != nullptr, [&](auto clean) {
        cut_clips_kernel<decltype(clean)::value><<<dim3((L + PC_CHUNK - 1) / PC_CHUNK, C), 256, 0, st>>>(src, start, L, ceiling ? *ceiling : 0.f, out);
    });
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}

// grid (Q), 256 threads: workgroup q owns samples [c0, c1) of chunk rt.chunk[q] of the RECORDING and walks spans [k0[q], k1[q]) per
// sample -- patch_compose_kernel's blend path on the recording's own sample axis (q is workgroup-uniform: the table arrives through
// scalar loads).  The spans of a chunk may belong to different contexts; each carries its own span_lim (where its context's generated
// audio ends) and, through its window, its own gain.  A sample of weight 0 is NOT written: out / pcm hold the caller's copy of the
// recording there, so the untouched chunks -- nearly all of a long recording -- cost nothing.  The written samples are
// patch_compose_kernel's, rounding for rounding: gain * gen; then that product (w == 1) or fma(w, g, (1 - w) * orig).  orig is the
// recording, never out.  The C ABI checked on the host copy that every region lies inside its window's row and inside [0, N22).
__global__ __launch_bounds__(256) void patch_regions_kernel(const float* __restrict__ orig, SiRegions rt, const float* __restrict__ gen, int Lrow,
                                                            const float* __restrict__ gain, int N22, float* __restrict__ out, int16_t* __restrict__ pcm) {
    const int q = blockIdx.x;
    const int c0 = rt.chunk[q] * PC_CHUNK, c1 = min(c0 + PC_CHUNK, N22);
    const int k0 = rt.k0[q], k1 = rt.k1[q], fade = rt.fade;
    for (int m = c0 + threadIdx.x; m < c1; m += 256) {
        float w = 0.f;
        int win = 0;
        for (int k = k0; k < k1; ++k) {                              // uniform loop: s, l, span_lim, span_win come through scalar loads
            if (m >= rt.span_lim[k]) continue;
            const int s = rt.start[k], l = rt.len[k];
            const int d = m - s;
            float wk = 0.f;
            if (d < 0) { if (d >= -fade) wk = rt.ramp[d + fade]; }
            else if (d < l) wk = 1.f;
            else if (d - l < fade) wk = rt.ramp[fade - 1 - (d - l)];
            if (wk > w) { w = wk; win = rt.span_win[k]; }
        }
        if (w == 0.f) continue;
        const float g0 = gain ? gain[rt.win_ctx[win]] : 1.f;
        const float g = __fmul_rn(g0, gen[(size_t)win * Lrow + (m - rt.win_start[win])]);
        const float v = w == 1.f ? g : __fmaf_rn(w, g, __fmul_rn(1.f - w, orig[m]));
        if (out) out[m] = v;
        if (pcm) pcm[m] = pc_pcm16(v);
    }
}

int si_launch_patch_regions(si_ctx* ctx, const float* orig, const SiRegions& rt, int Q, const float* gen, int Lrow, const float* gain,
                            int N22, float* out, int16_t* pcm, hipStream_t st) {
    if (Q <= 0) return SI_OK;
    si_prof_begin(ctx, "patch_regions", 0.0, (double)Q * PC_CHUNK * (8.0 + (out ? 4.0 : 0.0) + (pcm ? 2.0 : 0.0)), st);
    patch_regions_kernel<<<dim3(Q), 256, 0, st>>>(orig, rt, gen, Lrow, gain, N22, out, pcm);
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}
