// detect_kernels.hip -- dropout detection, gfx950: every maximal run of quiet samples (|x| <= thr) of at least min_len
// samples in a recording of up to 2^31 - 1 - 2048 samples, as (start, len) rows sorted by start.  One pass over the samples, the rest
// over one bit per sample and a few words per chunk of DT_CHUNK samples:
//   detect_bits_kernel     the quiet bits of a chunk (one byte per thread: 8 consecutive samples) + the chunk's summary {lead, trail}
//   detect_bits_ch_kernel  the same pass 1 over an INTERLEAVED recording: one channel of it, or all of them jointly
//   detect_peak*_kernel, detect_dead*_kernel  pass 0 and another pass 1: the bit means DEAD -- quiet against a threshold
//                          that follows the recording's peak, or held (equal to a neighbour) -- and the passes below do not care
//   detect_level_kernel    a third pass 1: the bit means that a window of low RMS level reaches over the sample
//   detect_burst_kernel    a fourth pass 1: the bit means that a window of LOUD second difference reaches over it
//   detect_invalid_kernel, detect_invalid_ch_kernel  a fifth pass 1: the bit means that the sample's VALUE is invalid
//   detect_impulse_kernel  a sixth pass 1: the bit means that a sample within `pad` of it has an AR prediction error far
//                          above that of its own neighbourhood; detect_impulse_residual_kernel writes that prediction error itself
//   detect_carry_kernel    carry[c] = the length of the quiet run that ends exactly in front of chunk c (a segmented scan, one workgroup)
//   detect_runs_kernel     <false>: the qualifying runs that END in each chunk, counted; <true>: written at offset[c] + rank
//   detect_offsets_kernel  the exclusive scan of the counts (one workgroup) and the total, a plain store
// A run belongs to the chunk its LAST sample lies in, chunks are numbered along the recording and the ranks inside a chunk follow the
// samples, so the rows come out sorted by construction: no atomics, no sort, and the same input gives the same bytes.
#include "common.h"
#include "detect_sizes.h"           // DT_CHUNK, DT_TILE and the launcher's host arithmetic: chunks, the scratch layout, the LDS request

struct DtMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct DtMin { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };
struct DtAdd { __device__ int operator()(int a, int b) const { return a + b; } };

// The EXCLUSIVE prefix of v over the workgroup's 256 threads under `op` (identity `ident`), and the workgroup's total in `tot`: a 6-step
// wave scan with shuffles, the four wave totals through LDS (sw: 4 ints).  Every thread of the workgroup calls it.
template <class Op>
__device__ __forceinline__ int dt_block_excl(int v, int ident, int* sw, int& tot, Op op) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl = op(u, incl);
    }
    if (lane == 63) sw[wave] = incl;
    __syncthreads();
    int pre = ident, all = ident;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int s = sw[w];
        if (w < wave) pre = op(pre, s);
        all = op(all, s);
    }
    tot = all;
    int ex = __shfl_up(incl, 1, 64);
    if (lane == 0) ex = ident;
    __syncthreads();                                                  // sw may be written again by the next call
    return op(pre, ex);
}

// NaN compares false: loud.  -0.0 has magnitude 0: quiet.  |-32768| is taken in int32 and is exact in fp32.
__device__ __forceinline__ bool dt_quiet(float v, float thr) { return __builtin_fabsf(v) <= thr; }
__device__ __forceinline__ bool dt_quiet(int16_t v, float thr) { const int a = v; return (float)(a < 0 ? -a : a) <= thr; }
// Packed 24-bit: thr counts 24-bit steps; |-2^23| is taken in int32 and is exact in fp32.
__device__ __forceinline__ bool dt_quiet(SiS24 v, float thr) { const int a = v.value(); return (float)(a < 0 ? -a : a) <= thr; }

// What pass 1 leaves per chunk, from the quiet bits b of this thread's eight samples (bits at and past len are 0, so the first loud bit
// is at most len): the bitmap byte, and through two workgroup scans the chunk's lead and trail.  Every thread of the workgroup calls it.
__device__ __forceinline__ void dt_store_chunk(unsigned b, int c, int len, uint8_t* __restrict__ bitmap, int32_t* __restrict__ lead,
                                               int32_t* __restrict__ trail, int* sw) {
    const int t = threadIdx.x;
    bitmap[(size_t)c * 256 + t] = (uint8_t)b;
    const unsigned loud = ~b & 0xffu;
    const int k = len - t * 8;
    const unsigned inside = loud & (k >= 8 ? 0xffu : k <= 0 ? 0u : (1u << k) - 1u);
    int first, last;
    (void)dt_block_excl(loud ? t * 8 + __builtin_ctz(loud) : DT_CHUNK, DT_CHUNK, sw, first, DtMin());
    (void)dt_block_excl(inside ? t * 8 + 31 - __builtin_clz(inside) : -1, -1, sw, last, DtMax());
    if (t == 0) {
        lead[c] = first;
        trail[c] = len - 1 - last;
    }
}

// This thread's eight consecutive samples of a one-channel chunk, for every pass 1 and pass 0: two / one 16-byte loads from an
// aligned base, else the chunk staged through LDS (tile: DT_CHUNK elements) with coalesced element loads.  Samples at and past n read 0.
// Every thread of the workgroup calls it.
template <typename T>
union DtEight { uint4 q[sizeof(T) / 2]; T e[8]; };

template <typename T>
__device__ __forceinline__ void dt_load_eight(const T* __restrict__ x, int n, int c0, int len, T* tile, DtEight<T>& u) {
    const int t = threadIdx.x, g = c0 + t * 8;
    if ((reinterpret_cast<size_t>(x) & 15) == 0) {
        if (g + 8 <= n) {
#pragma unroll
            for (int i = 0; i < (int)sizeof(T) / 2; ++i) u.q[i] = reinterpret_cast<const uint4*>(x + g)[i];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) u.e[j] = g + j < n ? x[g + j] : T(0);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = j * 256 + t;
            tile[i] = i < len ? x[c0 + i] : T(0);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < (int)sizeof(T) / 2; ++i) u.q[i] = reinterpret_cast<const uint4*>(tile + t * 8)[i];
    }
}

// The same for packed 24-bit samples.  The thread's eight samples are 24 bytes from byte 3 c0 + 24 t of the view, and
// 3 c0 is a multiple of 6144, so the alignment is again the call's: a base on the 8-byte grid takes three 8-byte loads; any other base
// stages the chunk through LDS, lane t on element t, t + 256, ... -- three byte loads each, which touch the sample's own bytes alone --
// and reads its 24 bytes from there (8-byte aligned in LDS: the tile is 16-byte aligned).  Samples at and past n read 0, and no byte
// at or past 3 n is loaded on either route.
// The eight samples leave the six loaded words by constant shifts (sample j = bytes [3 j, 3 j + 3) of the 24), so they stay in
// registers: a union with the words would be indexed by bytes and land in scratch or LDS.
template <>
union DtEight<SiS24> { SiS24 e[8]; };

__device__ __forceinline__ void dt_unpack_eight(const uint2 (&d)[3], DtEight<SiS24>& u) {
    const unsigned w[6] = {d[0].x, d[0].y, d[1].x, d[1].y, d[2].x, d[2].y};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = (3 * j) >> 2, sh = ((3 * j) & 3) * 8;           // sh = 0, 24, 16, 8: only 24 and 16 reach into the next word
        const unsigned v = sh > 8 ? w[k] >> sh | w[k + 1] << (32 - sh) : w[k] >> sh;
        u.e[j] = SiS24((int)v);                                       // keeps the low 24 bits
    }
}

__device__ __forceinline__ void dt_load_eight(const SiS24* __restrict__ x, int n, int c0, int len, SiS24* tile, DtEight<SiS24>& u) {
    const int t = threadIdx.x, g = c0 + t * 8;
    uint2 d[3];
    if ((reinterpret_cast<size_t>(x) & 7) == 0) {
        if (g + 8 <= n) {
#pragma unroll
            for (int i = 0; i < 3; ++i) d[i] = reinterpret_cast<const uint2*>(x + g)[i];
            dt_unpack_eight(d, u);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) u.e[j] = g + j < n ? x[g + j] : SiS24(0);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = j * 256 + t;
            tile[i] = i < len ? x[c0 + i] : SiS24(0);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = reinterpret_cast<const uint2*>(tile + t * 8)[i];
        dt_unpack_eight(d, u);
    }
}

// ------------------------------------------------------------------------------------------------ pass 1: bits + summary
// grid (chunks), 256 threads.  Thread t owns samples [c0 + 8 t, c0 + 8 t + 8): 32 bytes of fp32 (two 16-byte loads), 16 bytes of int16
// (one) or 24 bytes of packed 24-bit (three 8-byte loads; dt_load_eight above).  Callers pass views, so the base is generally off the 16-byte grid; c0 * sizeof(T) is a multiple of 16, so the alignment is the
// call's: an aligned call takes the 16-byte loads, any other stages the chunk through LDS with coalesced element loads and reads its
// eight samples from there.  Samples at and past n are loud, so bit (c0 + i >= n) is 0 and a run never reaches past the input.
//   lead  = quiet samples from the chunk's first sample forward (the chunk's length when all of it is quiet)
//   trail = quiet samples from the chunk's last sample backward (likewise)
template <typename T>
__global__ __launch_bounds__(256) void detect_bits_kernel(const T* __restrict__ x, int n, float thr, uint8_t* __restrict__ bitmap,
                                                          int32_t* __restrict__ lead, int32_t* __restrict__ trail) {
    __shared__ __attribute__((aligned(16))) T tile[DT_CHUNK];
    __shared__ int sw[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int c0 = c * DT_CHUNK, len = min(DT_CHUNK, n - c0);
    DtEight<T> u;
    dt_load_eight(x, n, c0, len, tile, u);
    unsigned b = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) b |= (t * 8 + j < len && dt_quiet(u.e[j], thr)) ? 1u << j : 0u;
    dt_store_chunk(b, c, len, bitmap, lead, trail, sw);
}

// The same pass over an INTERLEAVED recording: n sample times of ch channels, element i ch + channel.  A chunk is
// DT_CHUNK sample times = DT_CHUNK ch consecutive elements from element c0 ch on (a 64-bit offset; inside the chunk an int).
//   channel >= 0   sample time i is quiet iff that channel's element is: lane t loads times t, t + 256, ... (a stride of ch elements,
//                  which is what one channel of an interleaved file costs) and leaves one byte per time in LDS
//   channel  < 0   JOINT: quiet iff EVERY channel's element is.  Lane t loads elements t, t + 256, ... of the chunk -- consecutive
//                  lanes, consecutive elements, whatever ch is and wherever the base lies -- and leaves one byte per element in LDS;
//                  the thread that owns eight sample times then ANDs their 8 ch bytes (16 KB of LDS at ch = 8)
// Times at and past n are loud.  From the byte on this is detect_bits_kernel: the same bitmap, lead and trail (dt_store_chunk).
template <typename T>
__global__ __launch_bounds__(256) void detect_bits_ch_kernel(const T* __restrict__ x, int n, int ch, int channel, float thr,
                                                             uint8_t* __restrict__ bitmap, int32_t* __restrict__ lead, int32_t* __restrict__ trail) {
    __shared__ uint8_t sq[DT_CHUNK * SI_MAX_CHANNELS];
    __shared__ int sw[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int c0 = c * DT_CHUNK, len = min(DT_CHUNK, n - c0);
    const T* __restrict__ xc = x + (size_t)c0 * ch;
    unsigned b = 0;
    if (channel < 0) {
        const int cnt = len * ch;
        for (int e = t; e < DT_CHUNK * ch; e += 256) sq[e] = (e < cnt && dt_quiet(xc[e], thr)) ? 1 : 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            unsigned q = 1;
            for (int k = 0; k < ch; ++k) q &= sq[(t * 8 + j) * ch + k];
            b |= q << j;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = j * 256 + t;
            sq[i] = (i < len && dt_quiet(xc[(size_t)i * ch + channel], thr)) ? 1 : 0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) b |= (unsigned)sq[t * 8 + j] << j;
    }
    dt_store_chunk(b, c, len, bitmap, lead, trail, sw);
}

// ------------------------------------------------------------------------------------------------ pass 2: carries
// One workgroup.  Chunk c maps the quiet run that ends in front of it to the one that ends in front of chunk c + 1:
//     f_c(v) = v + len_c  when the whole chunk is quiet (lead == len_c),    f_c(v) = trail_c  otherwise
// a map (a, b): v -> a ? v + b : b, closed under composition ((a2, b2) after (a1, b1) = (a1 & a2, a2 ? b1 + b2 : b2)), so
// carry[c] = (f_{c-1} o ... o f_0)(0) is a scan.  Per tile of DT_TILE chunks a thread composes its 4 consecutive chunks, the
// workgroup scans the 256 maps (shuffles inside a wave, four wave totals through LDS), each thread applies its prefix to the tile's
// incoming carry and steps through its chunks; the tile's total map carries the value on.  b <= n throughout: no overflow.
struct DtMap { int a, b; };
__device__ __forceinline__ DtMap dt_then(DtMap p, DtMap q) { return DtMap{p.a & q.a, q.a ? p.b + q.b : q.b}; }   // q after p
__device__ __forceinline__ int dt_apply(DtMap m, int v) { return m.a ? v + m.b : m.b; }

__global__ __launch_bounds__(256) void detect_carry_kernel(const int32_t* __restrict__ lead, const int32_t* __restrict__ trail, int nchunks, int n,
                                                           int32_t* __restrict__ carry) {
    __shared__ DtMap sw[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int v0 = 0;                                                       // the carry into the tile (uniform)
    for (int base = 0; base < nchunks; base += DT_TILE) {
        DtMap f[4], mine{1, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = base + t * 4 + k;
            f[k] = DtMap{1, 0};
            if (c < nchunks) {
                const int len = min(DT_CHUNK, n - c * DT_CHUNK), ld = lead[c];
                f[k] = ld == len ? DtMap{1, len} : DtMap{0, trail[c]};
            }
            mine = dt_then(mine, f[k]);
        }
        DtMap incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            DtMap p{__shfl_up(incl.a, o, 64), __shfl_up(incl.b, o, 64)};
            if (lane >= o) incl = dt_then(p, incl);
        }
        if (lane == 63) sw[wave] = incl;
        __syncthreads();
        DtMap pre{1, 0}, all{1, 0};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const DtMap s = sw[w];
            if (w < wave) pre = dt_then(pre, s);
            all = dt_then(all, s);
        }
        DtMap ex{__shfl_up(incl.a, 1, 64), __shfl_up(incl.b, 1, 64)};
        if (lane == 0) ex = DtMap{1, 0};
        int v = dt_apply(dt_then(pre, ex), v0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = base + t * 4 + k;
            if (c < nchunks) carry[c] = v;
            v = dt_apply(f[k], v);
        }
        v0 = dt_apply(all, v0);
        __syncthreads();                                              // sw is written again by the next tile
    }
}

// ------------------------------------------------------------------------------------------------ passes 3 and 4: count, emit
// grid (chunks), 256 threads.  Sample i ends a run when it is quiet and sample i + 1 is loud (the chunk's last sample looks at the next
// chunk's first bit, lead[c + 1] > 0; past the last chunk everything is loud).  The run starts one past the last loud sample before i in
// the chunk -- inside the thread's own byte, or else the workgroup max-scan of "last loud position" over the bytes before it -- and, when
// the chunk has none, carry[c] samples before the chunk.  A thread's byte ends at most 4 runs; the exclusive sum of the qualifying ones
// over the workgroup is the rank of its first.  EMIT = false stores the chunk's count; EMIT = true stores rows offset[c] + rank that
// lie below max_runs, as plain stores.
template <bool EMIT>
__global__ __launch_bounds__(256) void detect_runs_kernel(const uint8_t* __restrict__ bitmap, const int32_t* __restrict__ lead,
                                                          const int32_t* __restrict__ carry, int nchunks, int min_len, int32_t* __restrict__ count,
                                                          const int32_t* __restrict__ offset, int32_t* __restrict__ runs, int max_runs) {
    __shared__ uint8_t sb[256];
    __shared__ int sw[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const unsigned b = bitmap[(size_t)c * 256 + t];
    sb[t] = (uint8_t)b;
    __syncthreads();
    const unsigned next = t < 255 ? sb[t + 1] & 1u : (c + 1 < nchunks && lead[c + 1] > 0) ? 1u : 0u;
    const unsigned ends = b & ~((b | next << 8) >> 1) & 0xffu;
    const unsigned loud = ~b & 0xffu;
    int unused;
    const int before = dt_block_excl(loud ? t * 8 + 31 - __builtin_clz(loud) : -1, -1, sw, unused, DtMax());
    const int c0 = c * DT_CHUNK, cin = carry[c];
    auto run_of = [&](int j, int& start) {                            // the run that ends at bit j of this thread's byte -> its length
        const unsigned below = loud & ((1u << j) - 1u);
        const int p = below ? t * 8 + 31 - __builtin_clz(below) : before;
        start = p >= 0 ? c0 + p + 1 : c0 - cin;
        return c0 + t * 8 + j - start + 1;
    };
    int m = 0;
    for (unsigned e = ends; e; e &= e - 1) {
        int start;
        m += run_of(__builtin_ctz(e), start) >= min_len ? 1 : 0;
    }
    int total;
    const int rank = dt_block_excl(m, 0, sw, total, DtAdd());
    if (!EMIT) {
        if (t == 0) count[c] = total;
    } else {
        int r = offset[c] + rank;
        for (unsigned e = ends; e; e &= e - 1) {
            int start;
            const int l = run_of(__builtin_ctz(e), start);
            if (l < min_len) continue;
            if (r < max_runs) {
                runs[2 * (size_t)r] = start;
                runs[2 * (size_t)r + 1] = l;
            }
            ++r;
        }
    }
}

// One workgroup: offset[c] = the counts of the chunks before c, and their total into *n_runs.  At most 1024 runs end in a chunk, so the
// total stays below 2^30 for every legal n.
__global__ __launch_bounds__(256) void detect_offsets_kernel(const int32_t* __restrict__ count, int nchunks, int32_t* __restrict__ offset,
                                                             int32_t* __restrict__ n_runs) {
    __shared__ int sw[4];
    const int t = threadIdx.x;
    int v0 = 0;
    for (int base = 0; base < nchunks; base += DT_TILE) {
        int f[4], mine = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = base + t * 4 + k;
            f[k] = c < nchunks ? count[c] : 0;
            mine += f[k];
        }
        int total;
        int v = v0 + dt_block_excl(mine, 0, sw, total, DtAdd());
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = base + t * 4 + k;
            if (c < nchunks) offset[c] = v;
            v += f[k];
        }
        v0 += total;
    }
    if (t == 0) *n_runs = v0;
}

// ------------------------------------------------------------------------------------------------ dead samples
// A richer pass 1 in front of the same passes 2 - 5: sample i is DEAD when it is quiet against a threshold that may follow the
// recording's peak, T = max(thr, rel * peak), or HELD -- equal to a neighbour of its own channel to within tol.
//   detect_peak_kernel / _ch   pass 0 (rel > 0 only): the largest finite magnitude of a chunk, one word per chunk
//   detect_peak_final_kernel   one workgroup: the largest of those words -> {peak, T} in two device words
//   detect_dead_kernel / _ch   pass 1: the dead bits of a chunk and its summary (dt_store_chunk)

// The magnitude of a sample as the bits of a non-negative finite float, which order as ints; NaN and +-inf count as 0 (skipped).
__device__ __forceinline__ int dt_mag_bits(float v) { const int b = __float_as_int(v) & 0x7fffffff; return b < 0x7f800000 ? b : 0; }
__device__ __forceinline__ int dt_mag_bits(int16_t v) { const int a = v; return __float_as_int((float)(a < 0 ? -a : a)); }
__device__ __forceinline__ int dt_mag_bits(SiS24 v) { const int a = v.value(); return __float_as_int((float)(a < 0 ? -a : a)); }      // 24-bit steps

// |a - b| <= tol.  fp32: one fp32 subtraction; a NaN neighbour and inf - inf compare false.  int16: the difference in int32 (65535 at most).
__device__ __forceinline__ bool dt_link(float a, float b, float tol) { return __builtin_fabsf(a - b) <= tol; }
__device__ __forceinline__ bool dt_link(int16_t a, int16_t b, float tol) { const int d = (int)a - (int)b; return (float)(d < 0 ? -d : d) <= tol; }
// packed 24-bit: the difference in int32, 2^24 - 1 at most and therefore exact in fp32; tol counts 24-bit steps
__device__ __forceinline__ bool dt_link(SiS24 a, SiS24 b, float tol) { const int d = a.value() - b.value(); return (float)(d < 0 ? -d : d) <= tol; }

__device__ __forceinline__ float dt_shfl_up1(float v) { return __shfl_up(v, 1, 64); }
__device__ __forceinline__ int16_t dt_shfl_up1(int16_t v) { return (int16_t)__shfl_up((int)v, 1, 64); }
__device__ __forceinline__ SiS24 dt_shfl_up1(SiS24 v) { return SiS24(__shfl_up(v.value(), 1, 64)); }
__device__ __forceinline__ float dt_shfl_down1(float v) { return __shfl_down(v, 1, 64); }
__device__ __forceinline__ SiS24 dt_shfl_down1(SiS24 v) { return SiS24(__shfl_down(v.value(), 1, 64)); }
__device__ __forceinline__ int16_t dt_shfl_down1(int16_t v) { return (int16_t)__shfl_down((int)v, 1, 64); }

// ------------------------------------------------------------------------------------------------ pass 0: the peak
// grid (chunks), 256 threads.  cpeak[c] = the largest dt_mag_bits over the chunk's samples below n (0 when none is finite).
template <typename T>
__global__ __launch_bounds__(256) void detect_peak_kernel(const T* __restrict__ x, int n, int32_t* __restrict__ cpeak) {
    __shared__ __attribute__((aligned(16))) T tile[DT_CHUNK];
    __shared__ int sw[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int c0 = c * DT_CHUNK, len = min(DT_CHUNK, n - c0);
    DtEight<T> u;
    dt_load_eight(x, n, c0, len, tile, u);
    int m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) m = max(m, t * 8 + j < len ? dt_mag_bits(u.e[j]) : 0);
    int top;
    (void)dt_block_excl(m, 0, sw, top, DtMax());
    if (t == 0) cpeak[c] = top;
}

// The same over an interleaved recording: a chunk is DT_CHUNK sample times.  channel >= 0: that channel's elements (a stride of ch);
// channel < 0: every element of the chunk, consecutive lanes on consecutive elements.
template <typename T>
__global__ __launch_bounds__(256) void detect_peak_ch_kernel(const T* __restrict__ x, int n, int ch, int channel, int32_t* __restrict__ cpeak) {
    __shared__ int sw[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int c0 = c * DT_CHUNK, len = min(DT_CHUNK, n - c0);
    const T* __restrict__ xc = x + (size_t)c0 * ch;
    int m = 0;
    if (channel < 0) {
        for (int e = t; e < len * ch; e += 256) m = max(m, dt_mag_bits(xc[e]));
    } else {
        for (int i = t; i < len; i += 256) m = max(m, dt_mag_bits(xc[(size_t)i * ch + channel]));
    }
    int top;
    (void)dt_block_excl(m, 0, sw, top, DtMax());
    if (t == 0) cpeak[c] = top;
}

// One workgroup: the largest per-chunk word, walked in tiles of DT_TILE chunks -> pk[0] = peak, pk[1] = T = max(thr, fl32(rel * peak)).
__global__ __launch_bounds__(256) void detect_peak_final_kernel(const int32_t* __restrict__ cpeak, int nchunks, float thr, float rel,
                                                                float* __restrict__ pk) {
    __shared__ int sw[4];
    const int t = threadIdx.x;
    int m = 0;
    for (int base = 0; base < nchunks; base += DT_TILE) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = base + t * 4 + k;
            if (c < nchunks) m = max(m, cpeak[c]);
        }
    }
    int top;
    (void)dt_block_excl(m, 0, sw, top, DtMax());
    if (t == 0) {
        const float peak = __int_as_float(top), prod = __fmul_rn(rel, peak);
        pk[0] = peak;
        pk[1] = thr > prod ? thr : prod;
    }
}

// ------------------------------------------------------------------------------------------------ pass 1: dead bits + summary
// grid (chunks), 256 threads, one channel.  Thread t owns samples [g, g + 8), g = c0 + 8 t, loaded as detect_bits_kernel loads them; it
// needs x[g - 1] and x[g + 8] as well: the neighbour lane's edge sample through a wave shuffle, and on lanes 0 and 63 of a wave (the
// wave's and the chunk's edges) one extra load each -- only when that sample exists, 0 <= index < n.  link(i) = |x[i] - x[i - 1]| <= tol
// exists for 1 <= i < n alone, so sample 0 has no left link, sample n - 1 no right one, and whatever lies in front of the base or
// behind the input is never read.  thr_dev, when given, holds T (pass 0); else T = thr.  Block 0 leaves T in *thr_out when asked.
template <typename T>
__global__ __launch_bounds__(256) void detect_dead_kernel(const T* __restrict__ x, int n, int kind, float thr, const float* __restrict__ thr_dev,
                                                          float tol, float* __restrict__ thr_out, uint8_t* __restrict__ bitmap,
                                                          int32_t* __restrict__ lead, int32_t* __restrict__ trail) {
    __shared__ __attribute__((aligned(16))) T tile[DT_CHUNK];
    __shared__ int sw[4];
    const int c = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const int c0 = c * DT_CHUNK, len = min(DT_CHUNK, n - c0), g = c0 + t * 8;
    const float Tq = thr_dev ? *thr_dev : thr;
    if (thr_out && c == 0 && t == 0) *thr_out = Tq;
    DtEight<T> u;
    dt_load_eight(x, n, c0, len, tile, u);
    T prev = dt_shfl_up1(u.e[7]), next = dt_shfl_down1(u.e[0]);
    if (lane == 0) prev = (g >= 1 && g - 1 < n) ? x[g - 1] : T(0);
    if (lane == 63) next = g + 8 < n ? x[g + 8] : T(0);
    unsigned lk = 0;                                                  // bit j: link(g + j), j = 0 .. 8
#pragma unroll
    for (int j = 0; j <= 8; ++j) {
        const T a = j == 0 ? prev : u.e[j - 1], b = j == 8 ? next : u.e[j];
        lk |= (g + j >= 1 && g + j < n && dt_link(b, a, tol)) ? 1u << j : 0u;
    }
    unsigned q = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) q |= (t * 8 + j < len && dt_quiet(u.e[j], Tq)) ? 1u << j : 0u;
    const unsigned held = (lk | lk >> 1) & 0xffu;                     // link(i) needs i < n, so no bit at or past len is set
    const unsigned b = ((kind & SI_DEAD_QUIET) ? q : 0u) | ((kind & SI_DEAD_HELD) ? held : 0u);
    dt_store_chunk(b, c, len, bitmap, lead, trail, sw);
}

// The same pass over an INTERLEAVED recording, through an image of the chunk in dynamic LDS with a one-sample-time halo on both sides:
// sample times c0 - 1 .. c0 + DT_CHUNK, (DT_CHUNK + 2) m elements, m = ch for the joint mode (every element of those times, consecutive
// lanes on consecutive elements) and 1 for one channel (that channel's elements).  A time outside [0, n) does not exist: it is not
// loaded, and a link to it is false.  Channel k's neighbours in the image are m elements away: elements (i +- 1) ch + k of the file,
// never the adjacent ones.  Joint: a time is dead when every channel's element is, each by its own links.
template <typename T>
__global__ __launch_bounds__(256) void detect_dead_ch_kernel(const T* __restrict__ x, int n, int ch, int channel, int kind, float thr,
                                                             const float* __restrict__ thr_dev, float tol, float* __restrict__ thr_out,
                                                             uint8_t* __restrict__ bitmap, int32_t* __restrict__ lead, int32_t* __restrict__ trail) {
    extern __shared__ __attribute__((aligned(16))) char dt_img[];
    __shared__ int sw[4];
    T* img = reinterpret_cast<T*>(dt_img);
    const int c = blockIdx.x, t = threadIdx.x;
    const int c0 = c * DT_CHUNK, len = min(DT_CHUNK, n - c0);
    const int m = channel < 0 ? ch : 1;
    const float Tq = thr_dev ? *thr_dev : thr;
    if (thr_out && c == 0 && t == 0) *thr_out = Tq;
    for (int e = t; e < (DT_CHUNK + 2) * m; e += 256) {
        const long time = (long)c0 - 1 + e / m;
        const bool exists = time >= 0 && time < n;
        img[e] = exists ? x[(size_t)time * ch + (channel < 0 ? e % m : channel)] : T(0);
    }
    __syncthreads();
    unsigned b = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = t * 8 + j, i = c0 + p;                          // image position p + 1
        const bool left = i >= 1 && i < n, right = i + 1 < n;         // link(i), link(i + 1) exist
        bool dead = p < len;
        for (int k = 0; k < m; ++k) {
            const T v = img[(p + 1) * m + k];
            const bool qt = (kind & SI_DEAD_QUIET) && dt_quiet(v, Tq);
            const bool hd = (kind & SI_DEAD_HELD) && ((left && dt_link(v, img[p * m + k], tol)) || (right && dt_link(img[(p + 2) * m + k], v, tol)));
            dead = dead && (qt || hd);
        }
        b |= dead ? 1u << j : 0u;
    }
    dt_store_chunk(b, c, len, bitmap, lead, trail, sw);
}

// ------------------------------------------------------------------------------------------------ windowed RMS level
// A third pass 1 in front of the same passes 2 - 5: sample j is DEAD when a window of low level reaches over it.  With h = half,
//   E(i)    = the sum of x[k]^2 over k in [max(0, i - h), min(n - 1, i + h)], float64, each square exact
//   low(i)  = no NaN or +-inf in that window, and E(i) <= fl64((T T) cnt(i)), cnt(i) the window's samples (truncated at both ends)
//   dead(j) = low(i) for some i in [j - h, j + h] inside [0, n): the union of the low windows
// A chunk needs low on [c0 - h, c0 + DT_CHUNK + h) and therefore samples on [c0 - 2 h, c0 + DT_CHUNK + 2 h): N = DT_CHUNK + 4 h squares,
// staged as float64 in dynamic LDS, lane t on element t.  A time outside [0, n) does not exist: it is not loaded, its square is 0
// (adding +0.0 to a sum of non-negative doubles changes nothing) and it is no `bad` sample; only cnt knows the truncation.
// NO WINDOW IS A DIFFERENCE OF RUNNING SUMS: behind one 3e38 sample a float64 prefix difference is garbage, and one NaN would poison
// every window after it.  The image is cut into segments of 2 h + 1 squares; P[p] sums its segment up to p, S[p] from p to the
// segment's end (two segmented scans, additions only), and the window [q, q + 2 h] is S[q] + P[q + 2 h] -- or the whole segment S[q]
// when it starts on one (van Herk's decomposition).  `bad` samples are counted with integers, whose prefix differences are exact; the
// dilation is an integer prefix count of low as well.
// LDS (cdna_hip_programming.md section 2): the staging and the window loops run lane t on element t + 256 k; the scans give a thread `per`
// consecutive elements with `per` ODD, so the 32 lanes of a ds_read_b64 group fall on 32 different bank pairs.
struct LvSeg { int f; double v; };   // a span of a segmented sum: v = the sum since the last segment head in it (all of it when f = 0)
__device__ __forceinline__ LvSeg lv_then(LvSeg p, LvSeg q) { return LvSeg{p.f | q.f, q.f ? q.v : p.v + q.v}; }   // q after p

__device__ __forceinline__ void lv_square(float v, double& s, int& bad) {
    const bool finite = (__float_as_int(v) & 0x7fffffff) < 0x7f800000;
    const double d = finite ? (double)v : 0.0;
    s = d * d;                                                        // 24 x 24 bits: exact
    bad = finite ? 0 : 1;
}
__device__ __forceinline__ void lv_square(int16_t v, double& s, int& bad) { const int a = v; s = (double)(a * a); bad = 0; }   // at most 2^30
__device__ __forceinline__ void lv_square(SiS24 v, double& s, int& bad) { const long a = v.value(); s = (double)(a * a); bad = 0; }    // at most 2^46: int64, exact in float64

// The square of the second difference d = a - 2 b + c of three consecutive samples of one channel, and whether any
// of the three is NaN or +-inf (the square is then staged as 0).
//   fp32: D = fl64(fl64((double)a + (double)c) - 2 (double)b), sq = fl64(D D): two roundings and one, in this order.  2 b is exact, so
//         a fused multiply-subtract for the second step would round the same value once; contraction is switched off all the same, and
//         the square goes to LDS before anything is added to it.
//   PCM:  d in int32 (|d| <= 131 070 for int16, < 2^26 for 24-bit), the square of two exact doubles: below 2^34 / 2^52, exact.
__device__ __forceinline__ void bu_square(float a, float b, float c, double& s, int& bad) {
#pragma clang fp contract(off)
    const bool finite = (__float_as_int(a) & 0x7fffffff) < 0x7f800000 && (__float_as_int(b) & 0x7fffffff) < 0x7f800000 &&
                        (__float_as_int(c) & 0x7fffffff) < 0x7f800000;
    const double sum = __dadd_rn((double)a, (double)c);
    const double D = __dsub_rn(sum, 2.0 * (double)b);
    s = finite ? __dmul_rn(D, D) : 0.0;
    bad = finite ? 0 : 1;
}
__device__ __forceinline__ void bu_square(int16_t a, int16_t b, int16_t c, double& s, int& bad) {
    const int d = (int)a - 2 * (int)b + (int)c;
    s = (double)d * (double)d;
    bad = 0;
}
__device__ __forceinline__ void bu_square(SiS24 a, SiS24 b, SiS24 c, double& s, int& bad) {
    const int d = a.value() - 2 * b.value() + c.value();
    s = (double)d * (double)d;
    bad = 0;
}

// dst[p] = the sum of src over p's segment up to p (REV = false: from the segment's first element; true: from p to its last).  Segments
// are [k L, (k + 1) L) cut at N.  Thread t walks `per` consecutive elements in scan order, the 256 partial sums are scanned with
// shuffles and four wave totals (sw), then it walks them again with its carry.  src == dst is fine.  Every thread calls it.
template <bool REV>
__device__ __forceinline__ void lv_seg_scan(const double* src, double* dst, int N, int per, int L, LvSeg* sw) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int u0 = min(t * per, N), u1 = min(u0 + per, N);
    LvSeg mine{0, 0.0};
    for (int u = u0; u < u1; ++u) {
        const int p = REV ? N - 1 - u : u;
        const bool head = REV ? p % L == L - 1 : p % L == 0;
        const double a = src[p];
        mine = head ? LvSeg{1, a} : LvSeg{mine.f, mine.v + a};
    }
    LvSeg incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const LvSeg p{__shfl_up(incl.f, o, 64), __shfl_up(incl.v, o, 64)};
        if (lane >= o) incl = lv_then(p, incl);
    }
    if (lane == 63) sw[wave] = incl;
    __syncthreads();
    LvSeg pre{0, 0.0};
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < wave) pre = lv_then(pre, sw[w]);
    LvSeg ex{__shfl_up(incl.f, 1, 64), __shfl_up(incl.v, 1, 64)};
    if (lane == 0) ex = LvSeg{0, 0.0};
    double run = lv_then(pre, ex).v;
    for (int u = u0; u < u1; ++u) {
        const int p = REV ? N - 1 - u : u;
        const bool head = REV ? p % L == L - 1 : p % L == 0;
        const double a = src[p];
        run = head ? a : run + a;
        dst[p] = run;
    }
    __syncthreads();                                                  // dst is read, and sw written again, after this
}

// a[p] = a[0] + ... + a[p], in place, integers.  Every thread calls it.
__device__ __forceinline__ void lv_count_scan(int* a, int N, int per, int* sw) {
    const int t = threadIdx.x;
    const int u0 = min(t * per, N), u1 = min(u0 + per, N);
    int mine = 0;
    for (int u = u0; u < u1; ++u) mine += a[u];
    int unused;
    int run = dt_block_excl(mine, 0, sw, unused, DtAdd());
    for (int u = u0; u < u1; ++u) {
        run += a[u];
        a[u] = run;
    }
    __syncthreads();
}

// grid (chunks), 256 threads, dynamic LDS 20 N + 4 M bytes (N = DT_CHUNK + 4 h squares, M = DT_CHUNK + 2 h windows; 139 264 at h = 1024).
// x is (n, ch) interleaved (ch = 1: one channel); channel >= 0 scans that channel, channel < 0 walks the channels one after another
// through the same image and ANDs their bits.  Element offsets are 64-bit.  thr_dev, when given, holds T (pass 0); else T = thr.
// BURST = false is the level detector above.  BURST = true stages the square of the second difference instead --
// centre k exists for 1 <= k <= n - 2 alone, its three samples x[k - 1], x[k], x[k + 1] come from global memory (neighbouring lanes,
// neighbouring elements: the second and third are cache hits, and the image has no room for a copy of the samples at h = 1024), a
// centre with a NaN or +-inf among the three is `bad` -- truncates the window to [1, n - 2], asks for cnt >= 1 and compares E >= lim.
template <typename T, bool BURST>
__device__ __forceinline__ void lv_window_body(const T* __restrict__ x, int n, int ch, int channel, int h, float thr,
                                               const float* __restrict__ thr_dev, float* __restrict__ thr_out,
                                               uint8_t* __restrict__ bitmap, int32_t* __restrict__ lead, int32_t* __restrict__ trail) {
    extern __shared__ __attribute__((aligned(16))) char lv_img[];
    __shared__ int sw[4];
    __shared__ LvSeg ssw[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int c0 = c * DT_CHUNK, len = min(DT_CHUNK, n - c0);
    const int N = DT_CHUNK + 4 * h, M = DT_CHUNK + 2 * h, L = 2 * h + 1;
    const int per = ((N + 255) / 256) | 1, perm = ((M + 255) / 256) | 1;
    double* P = reinterpret_cast<double*>(lv_img);                    // the squares, then their segment prefixes
    double* S = P + N;                                                // their segment suffixes
    int* bad = reinterpret_cast<int*>(S + N);                         // 1 at NaN / +-inf, then its prefix count
    int* low = bad + N;                                               // low(c0 - h + q), then its prefix count
    const float Tq = thr_dev ? *thr_dev : thr;
    if (thr_out && c == 0 && t == 0) *thr_out = Tq;
    const double T2 = (double)Tq * (double)Tq;                        // exact
    const int m = channel < 0 ? ch : 1;
    unsigned b = 0xffu;
    for (int k = 0; k < m; ++k) {
        const int col = channel < 0 ? k : channel;
        for (int p = t; p < N; p += 256) {
            const long time = (long)c0 - 2 * h + p;
            double s = 0.0;
            int bd = 0;
            if constexpr (BURST) {
                if (time >= 1 && time + 1 < n) {
                    const T* __restrict__ xk = x + (size_t)time * ch + col;
                    bu_square(*(xk - ch), *xk, *(xk + ch), s, bd);
                }
            } else {
                if (time >= 0 && time < n) lv_square(x[(size_t)time * ch + col], s, bd);
            }
            P[p] = s;
            bad[p] = bd;
        }
        __syncthreads();
        lv_seg_scan<true>(P, S, N, per, L, ssw);
        lv_seg_scan<false>(P, P, N, per, L, ssw);
        lv_count_scan(bad, N, per, sw);
        for (int q = t; q < M; q += 256) {
            const long i = (long)c0 - h + q;                          // the window's centre; its squares are image positions [q, q + 2 h]
            int lo = 0;
            if (i >= 0 && i < n) {
                const double E = q % L == 0 ? S[q] : S[q] + P[q + 2 * h];
                const int nb = bad[q + 2 * h] - (q > 0 ? bad[q - 1] : 0);
                if constexpr (BURST) {
                    const long a = i - h > 1 ? i - h : 1, z = i + h < n - 2 ? i + h : n - 2;      // z - a + 1 <= 0: no centre in the window
                    const double lim = __dmul_rn(T2, (double)(z - a + 1));
                    lo = (nb == 0 && z >= a && E >= lim) ? 1 : 0;
                } else {
                    const long a = i - h > 0 ? i - h : 0, z = i + h < n - 1 ? i + h : n - 1;
                    const double lim = __dmul_rn(T2, (double)(z - a + 1));
                    lo = (nb == 0 && E <= lim) ? 1 : 0;
                }
            }
            low[q] = lo;
        }
        __syncthreads();
        lv_count_scan(low, M, perm, sw);
        unsigned bk = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = t * 8 + j;                                  // low on times [c0 + r - h, c0 + r + h] = positions [r, r + 2 h]
            const int cnt = low[r + 2 * h] - (r > 0 ? low[r - 1] : 0);
            bk |= (r < len && cnt > 0) ? 1u << j : 0u;
        }
        b &= bk;
        __syncthreads();                                              // the next channel stages over the image
    }
    dt_store_chunk(b, c, len, bitmap, lead, trail, sw);
}

template <typename T>
__global__ __launch_bounds__(256) void detect_level_kernel(const T* __restrict__ x, int n, int ch, int channel, int h, float thr,
                                                           const float* __restrict__ thr_dev, float* __restrict__ thr_out,
                                                           uint8_t* __restrict__ bitmap, int32_t* __restrict__ lead, int32_t* __restrict__ trail) {
    lv_window_body<T, false>(x, n, ch, channel, h, thr, thr_dev, thr_out, bitmap, lead, trail);
}

// ------------------------------------------------------------------------------------------------ second-difference level
// A fourth pass 1: sample j is DEAD when a window whose second difference d(k) = x[k - 1] - 2 x[k] + x[k + 1] is LOUD reaches over it --
// a block of corrupted PCM (random data, swapped or misaligned bytes) is white at full scale, speech is not.  With h = half,
//   E(i)    = the sum of d(k)^2 over k in W(i) = [max(1, i - h), min(n - 2, i + h)], float64, additions only; cnt(i) = |W(i)|, maybe 0
//   hot(i)  = cnt(i) >= 1, no NaN or +-inf among the samples of W(i)'s differences, and E(i) >= fl64((T T) cnt(i))
//   dead(j) = hot(i) for some i in [j - h, j + h] inside [0, n)
// The image, the scans and the dilation are detect_level_kernel's (lv_window_body); a chunk reads samples [c0 - 2 h - 1, c0 + DT_CHUNK +
// 2 h + 1) cut to [0, n).  Grid, threads and dynamic LDS are detect_level_kernel's too.
template <typename T>
__global__ __launch_bounds__(256) void detect_burst_kernel(const T* __restrict__ x, int n, int ch, int channel, int h, float thr,
                                                           const float* __restrict__ thr_dev, float* __restrict__ thr_out,
                                                           uint8_t* __restrict__ bitmap, int32_t* __restrict__ lead, int32_t* __restrict__ trail) {
    lv_window_body<T, true>(x, n, ch, channel, h, thr, thr_dev, thr_out, bitmap, lead, trail);
}

// ------------------------------------------------------------------------------------------------ invalid samples
// A fifth pass 1: sample i is DEAD when its VALUE is the damage -- si_invalid(x[i], ceiling) (common.h): NaN of any payload, +-inf,
// |x| > ceiling; a PCM sample only under a finite ceiling, in the file's own steps.  Nothing looks at a neighbour, so the pass is
// detect_bits_kernel's with the other predicate: grid (chunks), 256 threads, dt_load_eight on either alignment route (the 24-bit routes
// included), the bits masked by t 8 + j < len -- a sample at or past n is never dead, whatever lies there -- then dt_store_chunk.
template <typename T>
__global__ __launch_bounds__(256) void detect_invalid_kernel(const T* __restrict__ x, int n, float ceiling, uint8_t* __restrict__ bitmap,
                                                             int32_t* __restrict__ lead, int32_t* __restrict__ trail) {
    __shared__ __attribute__((aligned(16))) T tile[DT_CHUNK];
    __shared__ int sw[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int c0 = c * DT_CHUNK, len = min(DT_CHUNK, n - c0);
    DtEight<T> u;
    dt_load_eight(x, n, c0, len, tile, u);
    unsigned b = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) b |= (t * 8 + j < len && si_invalid(u.e[j], ceiling)) ? 1u << j : 0u;
    dt_store_chunk(b, c, len, bitmap, lead, trail, sw);
}

// The same pass over an INTERLEAVED recording, shaped like detect_bits_ch_kernel and without a halo: channel >= 0 judges that channel's
// element of a sample time (never the adjacent one), channel < 0 is JOINT -- a time is dead when EVERY channel's element is invalid.
template <typename T>
__global__ __launch_bounds__(256) void detect_invalid_ch_kernel(const T* __restrict__ x, int n, int ch, int channel, float ceiling,
                                                                uint8_t* __restrict__ bitmap, int32_t* __restrict__ lead, int32_t* __restrict__ trail) {
    __shared__ uint8_t sq[DT_CHUNK * SI_MAX_CHANNELS];
    __shared__ int sw[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int c0 = c * DT_CHUNK, len = min(DT_CHUNK, n - c0);
    const T* __restrict__ xc = x + (size_t)c0 * ch;
    unsigned b = 0;
    if (channel < 0) {
        const int cnt = len * ch;
        for (int e = t; e < DT_CHUNK * ch; e += 256) sq[e] = (e < cnt && si_invalid(xc[e], ceiling)) ? 1 : 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            unsigned q = 1;
            for (int k = 0; k < ch; ++k) q &= sq[(t * 8 + j) * ch + k];
            b |= q << j;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = j * 256 + t;
            sq[i] = (i < len && si_invalid(xc[(size_t)i * ch + channel], ceiling)) ? 1 : 0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) b |= (unsigned)sq[t * 8 + j] << j;
    }
    dt_store_chunk(b, c, len, bitmap, lead, trail, sw);
}

// ------------------------------------------------------------------------------------------------ impulses
// A sixth pass 1: sample j is DEAD when a sample within `pad` of it is HOT -- its squared AR prediction error stands `ratio`^2 over the
// mean squared prediction error of its own neighbourhood.  For one channel, p = order, h = half, g = guard, blocks of IM_BLOCK = 512:
//   model of block b   fitted to F_b = [max(0, 512 b - 256), min(n, 512 (b + 1) + 256)): r[k] = sum of w[t] w[t + k] over F_b, k = 0 .. p, AS
//                      IM_PARTS = 8 INTERLEAVED PARTIAL SUMS (partial q takes t = q, q + 8, ... counted from F_b's first sample, in index
//                      order, from +0.0) ADDED IN ORDER q = 0 .. 7; r[0] *= 1 + 1e-9; Levinson-Durbin as mend_kernels.hip runs it; the model
//                      is (1, 0, ..., 0) when |F_b| <= p, r[0] == 0, or E <= 0 / non-finite at any step
//   badblk(b)          a NaN or +-inf lies in F_b (an integer count): every sample of the block is `bad`
//   e(t), p <= t < n   a_0 x[t] + a_1 x[t - 1] + ... + a_p x[t - p], added in this order, float64, nothing contracted; sq = fl64(e e)
//   L(t), R(t)         [max(p, t - h), t - g - 1] and [t + g + 1, min(n - 1, t + h)]; cnt = |L| + |R|; S = the sum of sq over both, BY
//                      ADDITIONS ONLY (two segmented scans with segments of h - g squares: a window is a suffix plus a prefix)
//   hot(t)             t >= p, cnt >= h - g, no bad sample at t or in L or R, sq > T T, fl64(sq cnt) > fl64(fl64(ratio ratio) S)
// The workgroup of chunk c fits the chunk's four blocks and `halo` = ceil((h + pad) / 512) blocks on either side (blocks outside the file
// do not exist), so every residual its windows and its dilation reach comes from the model of the residual's own block, whichever
// chunk computes it: the halo fits are redundant, not approximate.  Dynamic LDS: detect_sizes.h, dt_impulse_lds (135 168 bytes at halo 2).
// LDS reads of 8 bytes (cdna_hip_programming.md section 2): the staging, the residual and the window loops run lane t on element
// t + 256 k; the lag sums give eight consecutive lanes eight consecutive elements and the same second operand to each lag's eight; the
// scans are lv_seg_scan / lv_count_scan with an odd `per`.
struct ImBlock { int lo, hi, state; };                               // a block's fit window as image positions [lo, hi), and IM_*
constexpr int IM_FIT = 0, IM_NONE = 1, IM_BAD = 2;

__device__ __forceinline__ void im_stage(float v, double& d, int& nf) {
    const bool finite = (__float_as_int(v) & 0x7fffffff) < 0x7f800000;
    d = finite ? (double)v : 0.0;
    nf = finite ? 0 : 1;
}
__device__ __forceinline__ void im_stage(int16_t v, double& d, int& nf) { d = (double)v; nf = 0; }
__device__ __forceinline__ void im_stage(SiS24 v, double& d, int& nf) { d = (double)v.value(); nf = 0; }

// The residuals of chunk c's blocks and of `halo` blocks on either side, for column `col` of the (n, ch) file: E[i] = e(q0 + i) for
// image position i in [0, NQ), q0 = c0 - 512 halo, and 0.0 where there is none (a time outside [p, n), a bad block); bad[i] = 1 where
// p <= time < n lies in a bad block.  X (NX doubles), E (NQ), part (NQ) and ints (2 NQ words; bad = ints) are the regions of
// dt_impulse_lds.  Every thread of the workgroup calls it; it ends behind a barrier.
template <typename T>
__device__ __forceinline__ void im_residual_body(const T* __restrict__ x, int n, int ch, int col, int c0, int halo, int p, double* X, double* E,
                                                 double* part, int* ints, int* sw) {
#pragma clang fp contract(off)
    __shared__ double a[IM_MAX_BLOCKS][IM_MAX_ORDER + 1], r[IM_MAX_BLOCKS][IM_MAX_ORDER + 1];
    __shared__ ImBlock blk[IM_MAX_BLOCKS];
    const int t = threadIdx.x;
    const int NB = DT_CHUNK / IM_BLOCK + 2 * halo, NQ = dt_impulse_nq(halo), NX = dt_impulse_nx(halo);
    const long q0 = (long)c0 - (long)IM_BLOCK * halo, x0 = q0 - IM_WING;          // the times of E[0] and X[0]
    int* nf = ints;
    // ---- the samples as float64, a non-finite one as 0.0 and counted; a time outside [0, n) does not exist and is not loaded
    for (int i = t; i < NX; i += 256) {
        const long time = x0 + i;
        double v = 0.0;
        int f = 0;
        if (time >= 0 && time < n) im_stage(x[(size_t)time * ch + col], v, f);
        X[i] = v;
        nf[i] = f;
    }
    __syncthreads();
    lv_count_scan(nf, NX, ((NX + 255) / 256) | 1, sw);
    if (t < NB) {
        const long b0 = q0 + (long)IM_BLOCK * t;                      // the block's first time; its fit window starts at image position 512 t
        ImBlock k{0, 0, IM_NONE};
        if (b0 >= 0 && b0 < n) {
            k.lo = IM_BLOCK * t + (b0 < IM_WING ? IM_WING - (int)b0 : 0);
            k.hi = IM_BLOCK * t + 2 * IM_WING + IM_BLOCK - (b0 + IM_BLOCK + IM_WING > n ? (int)(b0 + IM_BLOCK + IM_WING - n) : 0);
            k.state = nf[k.hi - 1] - (k.lo > 0 ? nf[k.lo - 1] : 0) > 0 ? IM_BAD : IM_FIT;
        }
        blk[t] = k;
    }
    __syncthreads();
    // ---- r[k] of every block that is fitted: IM_PARTS interleaved partial sums per lag, each by one thread in index order
    for (int task = t; task < NB * (p + 1) * IM_PARTS; task += 256) {
        const int sub = task % IM_PARTS, k = task / IM_PARTS % (p + 1), b = task / (IM_PARTS * (p + 1));
        const ImBlock f = blk[b];
        double acc = 0.0;
        if (f.state == IM_FIT)
            for (int i = f.lo + sub; i + k < f.hi; i += IM_PARTS) acc = acc + X[i] * X[i + k];
        part[task] = acc;
    }
    __syncthreads();
    // ---- Levinson-Durbin, one thread per block
    if (t < NB && blk[t].state == IM_FIT) {
        double* rr = r[t];
        double* aa = a[t];
        const double* pt = part + (size_t)t * (p + 1) * IM_PARTS;
        for (int k = 0; k <= p; ++k) {
            double acc = pt[k * IM_PARTS];
            for (int q = 1; q < IM_PARTS; ++q) acc = acc + pt[k * IM_PARTS + q];
            rr[k] = acc;
            aa[k] = 0.0;
        }
        rr[0] = rr[0] * (1.0 + 1e-9);
        aa[0] = 1.0;
        bool delta = blk[t].hi - blk[t].lo <= p || rr[0] == 0.0;
        if (!delta) {
            double Ev = rr[0];
            for (int i = 1; i <= p; ++i) {
                double acc = rr[i];
                for (int j = 1; j < i; ++j) acc = acc + aa[j] * rr[i - j];
                const double kap = -acc / Ev;
                for (int j = 1; 2 * j <= i; ++j) {
                    const double lo = aa[j] + kap * aa[i - j], hi = aa[i - j] + kap * aa[j];
                    aa[j] = lo;
                    aa[i - j] = hi;
                }
                aa[i] = kap;
                Ev = Ev * (1.0 - kap * kap);
                if (!(Ev > 0.0) || !(Ev <= __DBL_MAX__)) { delta = true; break; }
            }
        }
        if (delta) {
            aa[0] = 1.0;
            for (int k = 1; k <= p; ++k) aa[k] = 0.0;
        }
    }
    __syncthreads();
    // ---- the residuals: x[t - j] in front of the block are the file's samples, staged with the rest (j <= p <= IM_WING)
    int* bad = ints;
    for (int i = t; i < NQ; i += 256) {
        const long time = q0 + i;
        const int b = i / IM_BLOCK;
        double e = 0.0;
        int bd = 0;
        if (time >= p && time < n) {
            if (blk[b].state == IM_BAD) bd = 1;
            else {
                const double* aa = a[b];
                const double* xt = X + i + IM_WING;
                double acc = aa[0] * xt[0];
                for (int j = 1; j <= p; ++j) acc = acc + aa[j] * xt[-j];
                e = acc;
            }
        }
        E[i] = e;
        bad[i] = bd;
    }
    __syncthreads();
}

// grid (chunks), 256 threads, dynamic LDS dt_impulse_lds(halo).bytes, halo = dt_impulse_halo(h, pad).  x is (n, ch) interleaved (ch = 1: one
// channel); channel >= 0 scans that channel, channel < 0 walks the channels one after another through the same image and ANDs their
// bits.  Element offsets are 64-bit.  thr_dev, when given, holds T (pass 0); else T = thr.  Block 0 leaves T in *thr_out when asked.
template <typename T>
__global__ __launch_bounds__(256) void detect_impulse_kernel(const T* __restrict__ x, int n, int ch, int channel, int p, int h, int g, int pad,
                                                             float ratio, float thr, const float* __restrict__ thr_dev, float* __restrict__ thr_out,
                                                             uint8_t* __restrict__ bitmap, int32_t* __restrict__ lead, int32_t* __restrict__ trail) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char im_img[];
    __shared__ int sw[4];
    __shared__ LvSeg ssw[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int c0 = c * DT_CHUNK, len = min(DT_CHUNK, n - c0);
    const int halo = dt_impulse_halo(h, pad), NQ = dt_impulse_nq(halo), base = IM_BLOCK * halo, wlen = h - g;
    const int per = ((NQ + 255) / 256) | 1;
    const DtImpulseLds at = dt_impulse_lds(halo);
    double* X = reinterpret_cast<double*>(im_img + at.x);             // the samples, then S: the segment suffixes of the squares
    double* E = reinterpret_cast<double*>(im_img + at.e);             // the residuals, then their squares
    double* P = reinterpret_cast<double*>(im_img + at.p);             // the lag partial sums, then the segment prefixes of the squares
    int* bad = reinterpret_cast<int*>(im_img + at.ints);              // 1 at a bad sample, then its prefix count
    int* hot = bad + NQ;                                              // hot(q0 + i), then its prefix count
    double* S = X;
    const float Tq = thr_dev ? *thr_dev : thr;
    if (thr_out && c == 0 && t == 0) *thr_out = Tq;
    const double T2 = (double)Tq * (double)Tq, R2 = (double)ratio * (double)ratio;    // both exact
    const long q0 = (long)c0 - base;
    const int m = channel < 0 ? ch : 1;
    unsigned b = 0xffu;
    for (int k = 0; k < m; ++k) {
        im_residual_body(x, n, ch, channel < 0 ? k : channel, c0, halo, p, X, E, P, bad, sw);
        for (int i = t; i < NQ; i += 256) E[i] = E[i] * E[i];
        __syncthreads();
        lv_seg_scan<true>(E, S, NQ, per, wlen, ssw);
        lv_seg_scan<false>(E, P, NQ, per, wlen, ssw);
        lv_count_scan(bad, NQ, per, sw);
        for (int i = t; i < NQ; i += 256) {
            const long time = q0 + i;
            int ht = 0;
            if (i >= base - pad && i < base + DT_CHUNK + pad && time >= p && time < n) {
                const int ql = i - h, qr = i + g + 1;                 // the two windows are positions [ql, i - g - 1] and [qr, i + h]
                const double sl = ql % wlen == 0 ? S[ql] : S[ql] + P[ql + wlen - 1];
                const double sr = qr % wlen == 0 ? S[qr] : S[qr] + P[qr + wlen - 1];
                const double sum = sl + sr;
                const long la = time - h > p ? time - h : p, rz = time + h < (long)n - 1 ? time + h : (long)n - 1;
                const long cl = time - g - la > 0 ? time - g - la : 0, cr = rz - time - g > 0 ? rz - time - g : 0;
                const int nb = (bad[i] - bad[i - 1]) + (bad[i - g - 1] - (ql > 0 ? bad[ql - 1] : 0)) + (bad[i + h] - bad[i + g]);
                const double sq = E[i], cnt = (double)(cl + cr);
                ht = (cl + cr >= wlen && nb == 0 && sq > T2 && sq * cnt > R2 * sum) ? 1 : 0;
            }
            hot[i] = ht;
        }
        __syncthreads();
        lv_count_scan(hot, NQ, per, sw);
        unsigned bk = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = base + t * 8 + j;                           // hot on times within pad = positions [i - pad, i + pad]
            const int cnt = hot[i + pad] - hot[i - pad - 1];
            bk |= (t * 8 + j < len && cnt > 0) ? 1u << j : 0u;
        }
        b &= bk;
        __syncthreads();                                              // the next channel stages over the image
    }
    dt_store_chunk(b, c, len, bitmap, lead, trail, sw);
}

// The whitened signal itself (si_impulse_residual): the same body with no halo, then e[c0 + i] = the residual of the chunk's sample i --
// 0.0 for a time below p, NaN for a bad sample.  grid (chunks), 256 threads, dynamic LDS dt_impulse_lds(0).bytes.
template <typename T>
__global__ __launch_bounds__(256) void detect_impulse_residual_kernel(const T* __restrict__ x, int n, int ch, int channel, int p,
                                                                      double* __restrict__ e) {
    extern __shared__ __attribute__((aligned(16))) char im_img[];
    __shared__ int sw[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int c0 = c * DT_CHUNK, len = min(DT_CHUNK, n - c0);
    const DtImpulseLds at = dt_impulse_lds(0);
    double* E = reinterpret_cast<double*>(im_img + at.e);
    int* bad = reinterpret_cast<int*>(im_img + at.ints);
    im_residual_body(x, n, ch, channel, c0, 0, p, reinterpret_cast<double*>(im_img + at.x), E, reinterpret_cast<double*>(im_img + at.p), bad, sw);
    for (int i = t; i < len; i += 256) e[(size_t)c0 + i] = bad[i] ? __builtin_nan("") : E[i];
}

// ------------------------------------------------------------------------------------------------ launcher
size_t si_detect_scratch_bytes(int n) { return dt_scratch(n).bytes; }     // the bitmap, six words per chunk and {peak, T} (detect_sizes.h)

// The six routes of a detection call.  The caller checked every argument.  scratch: si_detect_scratch_bytes(n) bytes,
// 16-byte aligned.  channels = 0: x is one channel of n samples; channels >= 1: x is interleaved, n sample times of `channels` channels,
// and `channel` picks one of them or, below 0, all of them jointly.  d.route names pass 1 and d carries its parameters (common.h).
//   pass 0   the peak and {peak, T}, only when d.rel > 0: the routes with no peak-relative threshold leave rel at 0
//   pass 1   the route's own kernel -> the bitmap and each chunk's lead / trail words: the one switch below
//   2 - 5    carry, count, offsets and, when max_runs > 0, emit: the same launches for every route
template <typename T>
static int dt_launch_t(si_ctx* ctx, const T* x, int n, int channels, int channel, float thr, int min_len, int32_t* runs, int max_runs,
                       int32_t* n_runs, char* scratch, hipStream_t st, SiDetect d) {
    const int chunks = dt_chunks(n);
    const DtScratch at = dt_scratch(n);
    uint8_t* bitmap = reinterpret_cast<uint8_t*>(scratch + at.bitmap);
    int32_t* lead = reinterpret_cast<int32_t*>(scratch + at.lead);
    int32_t* trail = reinterpret_cast<int32_t*>(scratch + at.trail);
    int32_t* carry = reinterpret_cast<int32_t*>(scratch + at.carry);
    int32_t* count = reinterpret_cast<int32_t*>(scratch + at.count);
    int32_t* offset = reinterpret_cast<int32_t*>(scratch + at.offset);
    int32_t* cpeak = reinterpret_cast<int32_t*>(scratch + at.cpeak);
    float* pk = reinterpret_cast<float*>(scratch + at.pk);            // {peak, T}
    const double bits = (double)chunks * 256.0, sums = (double)chunks * 4.0;
    // a single channel still moves the whole 32- or 64-byte sectors its elements lie in: counted as the chunk's elements either way
    const double samples = (double)n * (channels ? channels : 1) * (double)sizeof(T);

    const float* thr_dev = nullptr;                                   // T on the device, for the passes behind a pass 0
    if (d.rel > 0.f) {
        si_prof_begin(ctx, "detect_peak", 0.0, samples + sums, st);
        if (channels == 0) {
            detect_peak_kernel<T><<<dim3(chunks), 256, 0, st>>>(x, n, cpeak);
        } else {
            detect_peak_ch_kernel<T><<<dim3(chunks), 256, 0, st>>>(x, n, channels, channel, cpeak);
        }
        si_prof_end(ctx, st);
        SI_HIP_CHECK(hipGetLastError());
        si_prof_begin(ctx, "detect_peak_final", 0.0, sums + 8.0, st);
        detect_peak_final_kernel<<<dim3(1), 256, 0, st>>>(cpeak, chunks, thr, d.rel, pk);
        si_prof_end(ctx, st);
        SI_HIP_CHECK(hipGetLastError());
        thr_dev = pk + 1;
    }

    // Pass 1.  The families are those of the first two routes: the lists of families are closed.  The windowed kernels
    // have no one-channel twin: they take the one-channel file as ch = 1, c = 0.
    const int ch = channels ? channels : 1, c = channels ? channel : 0;
    switch (d.route) {
    case SI_DET_QUIET:
        if (channels == 0) {
            si_prof_begin(ctx, "detect_bits", 0.0, samples + bits + 2.0 * sums, st);
            detect_bits_kernel<T><<<dim3(chunks), 256, 0, st>>>(x, n, thr, bitmap, lead, trail);
        } else {
            si_prof_begin(ctx, "detect_bits_ch", 0.0, samples + bits + 2.0 * sums, st);
            detect_bits_ch_kernel<T><<<dim3(chunks), 256, 0, st>>>(x, n, channels, channel, thr, bitmap, lead, trail);
        }
        break;
    case SI_DET_DEAD:
        if (channels == 0) {
            si_prof_begin(ctx, "detect_dead", 0.0, samples + bits + 2.0 * sums, st);
            detect_dead_kernel<T><<<dim3(chunks), 256, 0, st>>>(x, n, d.kind, thr, thr_dev, d.tol, d.thr_out, bitmap, lead, trail);
        } else {
            const size_t lds = dt_dead_ch_lds(channel < 0 ? channels : 1, sizeof(T));      // 65 600 bytes at 8 fp32 channels
            if (int rc = si_ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&detect_dead_ch_kernel<T>), lds)) return rc;
            si_prof_begin(ctx, "detect_dead", 0.0, samples + bits + 2.0 * sums, st);
            detect_dead_ch_kernel<T><<<dim3(chunks), 256, lds, st>>>(x, n, channels, channel, d.kind, thr, thr_dev, d.tol, d.thr_out, bitmap, lead, trail);
        }
        break;
    case SI_DET_LEVEL: {
        const size_t lds = dt_window_lds(d.half);                     // 139 264 bytes at half = SI_LEVEL_MAX_HALF
        if (int rc = si_ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&detect_level_kernel<T>), lds)) return rc;
        si_prof_begin(ctx, "detect_dead", 0.0, samples + bits + 2.0 * sums, st);
        detect_level_kernel<T><<<dim3(chunks), 256, lds, st>>>(x, n, ch, c, d.half, thr, thr_dev, d.thr_out, bitmap, lead, trail);
        break;
    }
    case SI_DET_BURST: {
        const size_t lds = dt_window_lds(d.half);                     // detect_level_kernel's image
        if (int rc = si_ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&detect_burst_kernel<T>), lds)) return rc;
        si_prof_begin(ctx, "detect_dead", 0.0, samples + bits + 2.0 * sums, st);
        detect_burst_kernel<T><<<dim3(chunks), 256, lds, st>>>(x, n, ch, c, d.half, thr, thr_dev, d.thr_out, bitmap, lead, trail);
        break;
    }
    case SI_DET_INVALID:                                              // never behind a pass 0; thr is not read
        if (channels == 0) {
            si_prof_begin(ctx, "detect_bits", 0.0, samples + bits + 2.0 * sums, st);
            detect_invalid_kernel<T><<<dim3(chunks), 256, 0, st>>>(x, n, d.ceiling, bitmap, lead, trail);
        } else {
            si_prof_begin(ctx, "detect_bits_ch", 0.0, samples + bits + 2.0 * sums, st);
            detect_invalid_ch_kernel<T><<<dim3(chunks), 256, 0, st>>>(x, n, channels, channel, d.ceiling, bitmap, lead, trail);
        }
        break;
    case SI_DET_IMPULSE: {
        const size_t lds = dt_impulse_lds(dt_impulse_halo(d.half, d.pad)).bytes;           // 135 168 bytes at half + pad = 1024
        if (int rc = si_ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&detect_impulse_kernel<T>), lds)) return rc;
        si_prof_begin(ctx, "detect_dead", 0.0, samples + bits + 2.0 * sums, st);
        detect_impulse_kernel<T><<<dim3(chunks), 256, lds, st>>>(x, n, ch, c, d.order, d.half, d.guard, d.pad, d.ratio, thr, thr_dev, d.thr_out, bitmap,
                                                                lead, trail);
        break;
    }
    default:
        return SI_EINVAL;                                             // no such route: nothing was launched
    }
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());

    si_prof_begin(ctx, "detect_carry", 0.0, 3.0 * sums, st);
    detect_carry_kernel<<<dim3(1), 256, 0, st>>>(lead, trail, chunks, n, carry);
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());

    si_prof_begin(ctx, "detect_count", 0.0, bits + 3.0 * sums, st);
    detect_runs_kernel<false><<<dim3(chunks), 256, 0, st>>>(bitmap, lead, carry, chunks, min_len, count, nullptr, nullptr, 0);
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());

    si_prof_begin(ctx, "detect_offsets", 0.0, 2.0 * sums, st);
    detect_offsets_kernel<<<dim3(1), 256, 0, st>>>(count, chunks, offset, n_runs);
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());

    if (max_runs > 0) {
        si_prof_begin(ctx, "detect_emit", 0.0, bits + 3.0 * sums, st);
        detect_runs_kernel<true><<<dim3(chunks), 256, 0, st>>>(bitmap, lead, carry, chunks, min_len, nullptr, offset, runs, max_runs);
        si_prof_end(ctx, st);
        SI_HIP_CHECK(hipGetLastError());
    }
    return SI_OK;
}

// channels = 1 is a one-channel file for every route but SI_DET_QUIET: its elements are the mono call's, and so are its kernels.
// si_quiet_runs_ch reaches detect_bits_ch_kernel at channels = 1, as it always did; si_quiet_runs passes channels = 0.
int si_launch_detect(si_ctx* ctx, const void* x, int fmt, int n, int channels, int channel, float thr, int min_len, int32_t* runs, int max_runs,
                     int32_t* n_runs, char* scratch, hipStream_t st, SiDetect d) {
    if (d.route != SI_DET_QUIET && channels < 2) channels = channel = 0;
    int rc = SI_OK;
    si_with_sample(fmt, [&](auto tag) {
        rc = dt_launch_t(ctx, static_cast<decltype(tag)>(x), n, channels, channel, thr, min_len, runs, max_runs, n_runs, scratch, st, d);
    });
    return rc;
}

// The residual of one channel (si_impulse_residual): one launch, no scratch.  channels = 1 is a one-channel file.
template <typename T>
static int im_residual_launch_t(si_ctx* ctx, const T* x, int n, int channels, int channel, int order, double* e, hipStream_t st) {
    const size_t lds = dt_impulse_lds(0).bytes;                       // 69 632 bytes
    const void* kern = reinterpret_cast<const void*>(&detect_impulse_residual_kernel<T>);
    if (int rc = si_ensure_dyn_lds(ctx, kern, lds)) return rc;
    si_prof_begin(ctx, "detect_dead", 0.0, (double)n * channels * (double)sizeof(T) + (double)n * 8.0, st);
    detect_impulse_residual_kernel<T><<<dim3(dt_chunks(n)), 256, lds, st>>>(x, n, channels, channel, order, e);
    si_prof_end(ctx, st);
    SI_HIP_CHECK(hipGetLastError());
    return SI_OK;
}

int si_launch_impulse_residual(si_ctx* ctx, const void* x, int fmt, int n, int channels, int channel, int order, double* e, hipStream_t st) {
    int rc = SI_OK;
    si_with_sample(fmt, [&](auto tag) { rc = im_residual_launch_t(ctx, static_cast<decltype(tag)>(x), n, channels, channel, order, e, st); });
    return rc;
}
