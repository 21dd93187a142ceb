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
