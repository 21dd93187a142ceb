// detcheck -- the host arithmetic of the detection launcher (csrc/detect_sizes.h: chunk count, scratch layout, LDS request) as a
// stand-alone host program, built with -fsanitize=address,undefined by `make -C speech_inpainting_amd/csrc detcheck`.  It needs no
// device and nothing preloaded.  Every layout is also WALKED: a host buffer of exactly `bytes` bytes is allocated and the first and
// last byte of each array, as the kernels index it, is written, so an array that reached past the buffer or into its neighbour would
// stop the run under ASan.  Exit status 0 when every case answers as expected.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "detect_sizes.h"
#include "si_hip.h"

static int g_cases = 0, g_bad = 0;
#define EXPECT(cond, ...)                                                                                        \
    do {                                                                                                         \
        ++g_cases;                                                                                               \
        if (!(cond)) {                                                                                           \
            ++g_bad;                                                                                             \
            printf("detcheck: %s:%d: %s: ", __FILE__, __LINE__, #cond);                                          \
            printf(__VA_ARGS__);                                                                                 \
            printf("\n");                                                                                        \
        }                                                                                                        \
    } while (0)

static const long MAX_REC = 0x7fffffffL - 2048;      // api.hip's SI_MAX_REC: the largest n a detection call accepts
static const size_t CU_LDS = 163840;                 // bytes of LDS per CU on gfx950

static void check_layout(int n, bool walk) {
    const size_t chunks = (size_t)dt_chunks(n);
    const DtScratch at = dt_scratch(n);
    EXPECT((long)chunks * DT_CHUNK >= n && ((long)chunks - 1) * DT_CHUNK < n, "n = %d: %zu chunks", n, chunks);
    const size_t off[9] = {at.bitmap, at.lead, at.trail, at.carry, at.count, at.offset, at.cpeak, at.pk, at.bytes};
    const size_t need[8] = {chunks * 256, chunks * 4, chunks * 4, chunks * 4, chunks * 4, chunks * 4, chunks * 4, 8};
    for (int k = 0; k < 8; ++k) {
        EXPECT(off[k] % 16 == 0, "n = %d: array %d at byte %zu is off the 16-byte grid", n, k, off[k]);
        EXPECT(off[k] + need[k] <= off[k + 1], "n = %d: array %d = [%zu, %zu) reaches past %zu", n, k, off[k], off[k] + need[k], off[k + 1]);
    }
    EXPECT(at.bytes == chunks * 256 + 6 * ((chunks * 4 + 15) / 16 * 16) + 16, "n = %d: %zu bytes", n, at.bytes);
    if (!walk) return;
    std::vector<unsigned char> buf(at.bytes);
    unsigned char* s = buf.data();
    s[at.bitmap] = 1, s[at.bitmap + (chunks - 1) * 256 + 255] = 1;                       // bitmap[c * 256 + t]
    for (size_t a : {at.lead, at.trail, at.carry, at.count, at.offset, at.cpeak}) {     // word[c]
        int32_t w = 7;
        memcpy(s + a, &w, 4), memcpy(s + a + (chunks - 1) * 4, &w, 4);
    }
    float pk[2] = {1.f, 2.f};
    memcpy(s + at.pk, pk, 8);
}

// The dynamic LDS of the impulse pass at half window h, dilation pad, order p and guard g, WALKED: a buffer of exactly
// dt_impulse_lds(halo).bytes, and the first and last element every loop of detect_impulse_kernel touches in each of its arrays.
static void check_impulse(int h, int pad, int p, int g) {
    const int halo = dt_impulse_halo(h, pad), NQ = dt_impulse_nq(halo), NX = dt_impulse_nx(halo), NB = DT_CHUNK / IM_BLOCK + 2 * halo;
    const DtImpulseLds at = dt_impulse_lds(halo);
    const int base = IM_BLOCK * halo, wlen = h - g;
    EXPECT(halo >= 0 && halo <= IM_MAX_HALO && NB <= IM_MAX_BLOCKS && base >= h + pad && wlen >= 1, "h = %d, pad = %d: halo %d", h, pad, halo);
    EXPECT(at.x == 0 && at.e == 8 * (size_t)NX && at.p == at.e + 8 * (size_t)NQ && at.ints == at.p + 8 * (size_t)NQ && at.bytes == at.ints + 8 * (size_t)NQ,
           "h = %d, pad = %d: the regions", h, pad);
    EXPECT(at.bytes == 32 * (size_t)NQ + 4096 && at.bytes + 8192 <= CU_LDS && at.ints % 8 == 0, "h = %d, pad = %d: %zu bytes", h, pad, at.bytes);
    EXPECT(NQ <= NX && NX <= 2 * NQ && NB * (p + 1) * IM_PARTS <= NQ, "h = %d, pad = %d, p = %d: S in X, nf in the words, the partial sums in P", h, pad, p);
    std::vector<unsigned char> buf(at.bytes);
    unsigned char* s = buf.data();
    const double d = 1.0;
    const int32_t w = 1;
    auto f64 = [&](size_t region, long i) { EXPECT(i >= 0, "index %ld", i); memcpy(s + region + 8 * (size_t)i, &d, 8); };
    auto i32 = [&](long i) { EXPECT(i >= 0, "index %ld", i); memcpy(s + at.ints + 4 * (size_t)i, &w, 4); };
    f64(at.x, 0), f64(at.x, NX - 1), i32(0), i32(NX - 1);                                  // the staged samples and their non-finite count
    f64(at.x, IM_BLOCK * (NB - 1) + 2 * IM_WING + IM_BLOCK - 1);                           // the last block's fit window ends with the image
    f64(at.p, 0), f64(at.p, (long)NB * (p + 1) * IM_PARTS - 1);                            // the lag partial sums
    f64(at.x, 0 + IM_WING - p), f64(at.x, NQ - 1 + IM_WING);                               // the residual's oldest and newest sample
    f64(at.e, 0), f64(at.e, NQ - 1), i32(NQ - 1);                                          // e / sq and bad
    for (long i : {(long)base - pad, (long)base + DT_CHUNK + pad - 1}) {                   // the first and last candidate of hot
        const long ql = i - h, qr = i + g + 1;
        f64(at.x, ql), f64(at.p, ql + wlen - 1), f64(at.x, qr), f64(at.p, qr + wlen - 1);  // S[ql], P[..], S[qr], P[..]; S lies over X
        EXPECT(qr + wlen - 1 == i + h && i + h <= NQ - 1 && ql >= 0, "h = %d, pad = %d: windows of position %ld", h, pad, i);
        i32(i - 1), i32(i - g - 1), i32(ql > 0 ? ql - 1 : 0), i32(i + h), i32(i + g);      // the prefix counts of bad
    }
    i32(NQ + 0), i32(NQ + NQ - 1);                                                         // hot
    i32(NQ + base - pad - 1), i32(NQ + base + DT_CHUNK - 1 + pad);                         // the dilation's first and last read
    EXPECT(base - pad - 1 >= 0 && base + DT_CHUNK - 1 + pad <= NQ - 1, "h = %d, pad = %d: the dilation", h, pad);
}

int main() {
    // the scratch layout: every n around the chunk and 16-byte-rounding seams, walked; the largest legal n, arithmetic only
    for (int n : {1, 2, 3, 7, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048, 4 * 2048, 4 * 2048 + 1, 5 * 2048 + 1, 1024 * 2048, 1024 * 2048 + 1,
                  1027 * 2048 - 3, 2 * 1024 * 2048 + 4101, 100000000})
        check_layout(n, true);
    for (long n = 1; n <= 70000; n += 13) check_layout((int)n, true);
    check_layout((int)MAX_REC, false);
    check_layout((int)MAX_REC - 2047, false);
    EXPECT(dt_chunks((int)MAX_REC) == 1048575, "%d chunks at the largest n", dt_chunks((int)MAX_REC));
    EXPECT(dt_scratch((int)MAX_REC).bytes == 1048575ul * 256 + 6 * 4194304ul + 16, "%zu bytes at the largest n", dt_scratch((int)MAX_REC).bytes);
    // the LDS request of the windowed passes
    size_t last = 0;
    for (int h = 0; h <= SI_LEVEL_MAX_HALF; ++h) {
        const size_t N = DT_CHUNK + 4 * (size_t)h, M = DT_CHUNK + 2 * (size_t)h, lds = dt_window_lds(h);
        EXPECT(lds == 2 * 8 * N + 4 * N + 4 * M, "h = %d: %zu bytes", h, lds);
        EXPECT(lds <= CU_LDS && lds > last && lds % 8 == 0, "h = %d: %zu bytes", h, lds);
        // the arrays as the kernel lays them out: P, S (float64 [N]), bad (int32 [N]), low (int32 [M]); the last index each loop touches
        const size_t P = 0, S = P + 8 * N, bad = S + 8 * N, low = bad + 4 * N;
        EXPECT(bad % 8 == 0 && low % 4 == 0 && low + 4 * M == lds, "h = %d", h);
        EXPECT((DT_CHUNK + 2 * (size_t)h - 1) + 2 * (size_t)h == N - 1, "h = %d: the last window's last square", h);      // q + 2 h, q = M - 1
        EXPECT((DT_CHUNK - 1) + 2 * (size_t)h == M - 1, "h = %d: the last sample's last window", h);                      // r + 2 h, r = DT_CHUNK - 1
        last = lds;
    }
    EXPECT(dt_window_lds(0) == 49152, "%zu", dt_window_lds(0));
    EXPECT(dt_window_lds(SI_LEVEL_MAX_HALF) == 139264, "%zu", dt_window_lds(SI_LEVEL_MAX_HALF));
    // an fp32 copy of the N + 2 samples beside the image does not fit, which is why there is none
    const size_t copy = 4 * (size_t)(DT_CHUNK + 4 * SI_LEVEL_MAX_HALF + 2);
    EXPECT(copy == 24584 && dt_window_lds(SI_LEVEL_MAX_HALF) + copy == 163848 && dt_window_lds(SI_LEVEL_MAX_HALF) + copy > CU_LDS, "%zu", copy);
    // the samples a chunk of the second-difference pass reads, [c0 - 2 h - 1, c0 + DT_CHUNK + 2 h + 1) cut to [0, n): centres 1 .. n - 2 only
    for (int n : {1, 2, 3, 4, 2049, 4101, (int)MAX_REC})
        for (int h : {0, 1, 1024}) {
            const int chunks = dt_chunks(n);
            for (int c : {0, chunks / 2, chunks - 1}) {
                const long c0 = (long)c * DT_CHUNK;
                long lo = n, hi = -1;
                for (long p : {0L, (long)DT_CHUNK + 4 * h - 1}) {                        // the image's first and last position
                    const long k = c0 - 2 * h + p;
                    if (k >= 1 && k + 1 < n) lo = k - 1 < lo ? k - 1 : lo, hi = k + 1 > hi ? k + 1 : hi;
                }
                EXPECT(hi < n && (hi < 0 || lo >= 0), "n = %d, h = %d, chunk %d: reads [%ld, %ld]", n, h, c, lo, hi);
            }
        }
    // the image of detect_dead_ch_kernel: every channel count the ABI accepts, joint (m = channels) or one channel (m = 1), in each sample
    // type, WALKED: the first element staged and the last one read, img[(p + 2) m + k] at p = DT_CHUNK - 1, k = m - 1
    for (size_t elem : {(size_t)4, (size_t)2, (size_t)3})
        for (int m = 1; m <= SI_MAX_CHANNELS; ++m) {
            const size_t lds = dt_dead_ch_lds(m, elem);
            EXPECT(lds == (size_t)(DT_CHUNK + 2) * m * elem && lds + 16 <= CU_LDS, "m = %d, %zu-byte samples: %zu bytes", m, elem, lds);
            std::vector<unsigned char> img(lds);
            const size_t last = (size_t)(DT_CHUNK - 1 + 2) * m + (m - 1);
            memset(img.data(), 1, elem), memset(img.data() + last * elem, 1, elem);
            EXPECT((last + 1) * elem == lds, "m = %d: the last element ends at byte %zu of %zu", m, (last + 1) * elem, lds);
        }
    EXPECT(dt_dead_ch_lds(8, 4) == 65600, "%zu", dt_dead_ch_lds(8, 4));
    // the impulse pass: every (half, pad, order, guard) at the limits, and every half in between at the extreme pads
    for (int p : {2, 16, SI_IMPULSE_MAX_ORDER})
        for (int g : {0, 4, SI_IMPULSE_MAX_GUARD})
            for (int pad : {0, 2, SI_IMPULSE_MAX_PAD})
                for (int h = g + 1; h + pad <= SI_IMPULSE_MAX_HALF; h += (h < 16 || h + pad > SI_IMPULSE_MAX_HALF - 16 || h % 512 > 500 || h % 512 < 12) ? 1 : 37)
                    check_impulse(h, pad, p, g);
    EXPECT(IM_MAX_ORDER == SI_IMPULSE_MAX_ORDER && IM_MAX_HALF == SI_IMPULSE_MAX_HALF && IM_MAX_GUARD == SI_IMPULSE_MAX_GUARD && IM_MAX_PAD == SI_IMPULSE_MAX_PAD,
           "detect_sizes.h against si_hip.h");
    EXPECT(dt_impulse_lds(0).bytes == 69632 && dt_impulse_lds(1).bytes == 102400 && dt_impulse_lds(2).bytes == 135168, "%zu", dt_impulse_lds(2).bytes);
    EXPECT(dt_impulse_halo(1, 0) == 1 && dt_impulse_halo(512, 0) == 1 && dt_impulse_halo(511, 2) == 2 && dt_impulse_halo(1008, 16) == 2 && IM_MAX_HALO == 2, "halo");
    // 135 168 bytes dynamic + 4 400 static (the models, the lag sums' r, the block table, the scan words) stay under the CU's LDS
    EXPECT(dt_impulse_lds(IM_MAX_HALO).bytes + 4400 <= CU_LDS, "%zu", dt_impulse_lds(IM_MAX_HALO).bytes + 4400);
    printf("detcheck: %d cases, %d answered as expected, %d not\n", g_cases, g_cases - g_bad, g_bad);
    return g_bad ? 1 : 0;
}
