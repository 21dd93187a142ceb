// detect_sizes.h -- the host arithmetic of the detection launcher (detect_kernels.hip): how many chunks a
// recording has, where each array of the detector's scratch lies, and how much dynamic LDS the windowed passes ask for.  Plain C++,
// no HIP header, so it also builds with a host compiler under sanitizers (tools/detcheck_main.cpp, the `detcheck` target).
#pragma once
#include <cstddef>
#include <cstdint>

constexpr int DT_CHUNK = 2048;      // samples per workgroup: 256 threads x 8 consecutive samples (patch_kernels.hip's PC_CHUNK)
constexpr int DT_TILE = 1024;       // chunks per tile of the two single-workgroup scans: 256 threads x 4 consecutive chunks

inline int dt_chunks(int n) { return (int)(((long)n + DT_CHUNK - 1) / DT_CHUNK); }

// The scratch of one detection call over n samples, as byte offsets from a 16-byte aligned base: the bitmap (one byte per eight
// samples), six int32 words per chunk (each array rounded up to 16 bytes) and {peak, T}.
struct DtScratch { size_t bitmap, lead, trail, carry, count, offset, cpeak, pk, bytes; };

inline DtScratch dt_scratch(int n) {
    const size_t chunks = (size_t)dt_chunks(n);
    const size_t words = (chunks * sizeof(int32_t) + 15) & ~(size_t)15;
    const size_t p = chunks * 256;
    return DtScratch{0, p, p + words, p + 2 * words, p + 3 * words, p + 4 * words, p + 5 * words, p + 6 * words, p + 6 * words + 16};
}

// The dynamic LDS of detect_level_kernel and detect_burst_kernel at half window h: two float64 arrays and an int32 array of N =
// DT_CHUNK + 4 h elements, an int32 array of M = DT_CHUNK + 2 h.  139 264 bytes at h = 1024 (SI_LEVEL_MAX_HALF).
inline size_t dt_window_lds(int h) { return 20 * (size_t)(DT_CHUNK + 4 * h) + 4 * (size_t)(DT_CHUNK + 2 * h); }

// The dynamic LDS of detect_dead_ch_kernel: the chunk's samples and one neighbour on either side, for each of the m channels it judges
// (all of them jointly, or one), in the file's own sample type of `elem` bytes.  65 600 bytes at 8 fp32 channels.
inline size_t dt_dead_ch_lds(int m, size_t elem) { return (size_t)(DT_CHUNK + 2) * (size_t)m * elem; }

// The impulse pass (detect_impulse_kernel, detect_impulse_residual_kernel).  A chunk is four model blocks of IM_BLOCK
// samples; a block's fit window reaches IM_WING samples past it on either side; the detector also fits `halo` blocks on either side of
// the chunk, enough for the widest window (half) and the dilation (pad) of the chunk's edge samples.  The residual tap has halo = 0.
constexpr int IM_BLOCK = 512, IM_WING = 256, IM_PARTS = 8;
constexpr int IM_MAX_ORDER = 32, IM_MAX_HALF = 1024, IM_MAX_GUARD = 64, IM_MAX_PAD = 16;   // SI_IMPULSE_MAX_* (si_hip.h)
constexpr int IM_MAX_HALO = (IM_MAX_HALF + IM_BLOCK - 1) / IM_BLOCK;                       // half + pad <= IM_MAX_HALF
constexpr int IM_MAX_BLOCKS = DT_CHUNK / IM_BLOCK + 2 * IM_MAX_HALO;                       // 8 models per workgroup at most

constexpr int dt_impulse_halo(int half, int pad) { return (half + pad + IM_BLOCK - 1) / IM_BLOCK; }
// the residual image of a workgroup: NQ = its blocks' samples; the staged samples: NX = NQ and a wing on either side
constexpr int dt_impulse_nq(int halo) { return DT_CHUNK + 2 * halo * IM_BLOCK; }
constexpr int dt_impulse_nx(int halo) { return dt_impulse_nq(halo) + 2 * IM_WING; }
// (constexpr, so that the kernels use the same arithmetic as the launcher.)
// Byte offsets into the dynamic LDS: the samples as float64 (NX; later the windows' segment suffixes, NQ), the residuals and then their
// squares (NQ), the lag partial sums (blocks * (order + 1) * IM_PARTS) and later the segment prefixes (NQ), and 2 NQ int32 words: the
// non-finite prefix count over the samples (NX) first, then the `bad` and `hot` images (NQ each).  135 168 bytes at halo = 2.
struct DtImpulseLds { size_t x, e, p, ints, bytes; };
constexpr DtImpulseLds dt_impulse_lds(int halo) {
    const size_t nq = (size_t)dt_impulse_nq(halo), nx = (size_t)dt_impulse_nx(halo);
    return DtImpulseLds{0, 8 * nx, 8 * (nx + nq), 8 * (nx + 2 * nq), 8 * (nx + 2 * nq) + 4 * 2 * nq};
}
