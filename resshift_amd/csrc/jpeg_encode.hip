// rs_jpeg_encode: a finished baseline JPEG FILE per image in device memory (include/resshift_hip.h "JPEG files"), byte for byte
// what libjpeg writes at 4:2:0 with the default tables: jpeg_codec.hip's forward path (jpeg_common.h), then the entropy stage that the codec
// never materialises - Huffman coding with the Annex K tables, byte stuffing, the header.  Everything is integer arithmetic and every step
// is a function of the image and its quality alone, so a batch is its B = 1 calls byte for byte.
//
// Launches, all on the caller's stream; NO kernel waits for another workgroup - a prefix sum that does not fit one workgroup is a reduce, a
// scan of the partial sums and a second pass (je_scan), never a look-back or a grid barrier:
//   1. je_transform   a workgroup per tile of 8 x 4 MCUs, the codec's mapping: colour into LDS, then a thread per 8 x 8 block with the block in
//                     registers: forward DCT, quantise, the 64 coefficients in zigzag order as int16 to the workspace, in scan order (per MCU
//                     Y00, Y01, Y10, Y11, Cb, Cr; MCUs row-major).  The Y blocks libjpeg never transforms (DUMMY blocks) are not written.
//   2. je_bits        a thread per block: its code bits.  je_block_dc has the DC rule (the difference against the previous block of the
//                     component, dummy blocks repeating the DC of the block before them), je_walk the symbols.
//   3. je_scan        exclusive prefix sum of the bits per image -> every block's bit offset, the image's bit count
//   4. je_zero        zeroes the words of the raw scan that the image will use
//   5. je_emit        a thread per block: je_walk again, the codes MSB first into big-endian 32-bit words at the block's offset, OR-ed in with
//                     vector atomics (neighbouring blocks share words)
//   6. je_count       a thread per 64 raw bytes: how many are 0xFF (the last byte padded with 1-bits first)
//   7. je_scan        exclusive prefix sum of those counts per image -> where every 64 bytes land in the file
//   8. je_write       a thread per 64 raw bytes: the bytes, 0x00 after every 0xFF; then EOI and nbytes[b]; one more workgroup per image
//                     writes the 623 header bytes.  Nothing at or beyond nbytes[b] is written.
#include "jpeg_common.h"
#include <climits>

constexpr int JE_THREADS = 256;
constexpr int JE_TX = 8, JE_TY = 4;                          // MCUs of a tile (the codec's)
constexpr int JE_YW = JE_TX * 16, JE_YH = JE_TY * 16, JE_YP = JE_YW + 8;
constexpr int JE_CW = JE_TX * 8, JE_CH = JE_TY * 8;
constexpr int JE_YBLOCKS = 4 * JE_TX * JE_TY, JE_CBLOCKS = JE_TX * JE_TY;
static_assert(JE_YBLOCKS + 2 * JE_CBLOCKS <= JE_THREADS, "a thread per block");
constexpr int JE_SCAN = 8 * JE_THREADS;                      // elements one workgroup scans
constexpr int JE_ELEM = 64;                                  // raw bytes of one element of the stuffing pass (16 words)
constexpr int JE_SCAN_OFFSET = 623;                          // the header's length
constexpr int JE_ROW = 33;                                   // LDS pitch, in words, of a block's 32 coefficient words (odd: no bank conflicts)

// natural index (8 u + v) of the k-th coefficient in zigzag order
constexpr int je_zigzag(int k) {
    constexpr unsigned char z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k];
}

// ---- Annex K.3: the number of codes of each length 1 .. 16, the symbols in code order ------------------------------------------------
struct JeSpec { unsigned char bits[16]; unsigned char vals[162]; int n; };
constexpr JeSpec JE_SPEC[4] = {   // in the order of the file's DHT segments: DC luminance, AC luminance, DC chrominance, AC chrominance
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
      0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
      0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
      0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
     162},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
      0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
      0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
      0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
     162},
};

// What the kernels read: the canonical codes (Annex C) as (length << 16) | code, indexed by symbol - dc[t][category], ac[t][run << 4 | category],
// t = 0 luminance, 1 chrominance, 0 where the table has no such symbol; the zigzag order; the header with the DQT payloads and the SOF0 size
// left zero (je_write fills them in).
struct JeTables {
    unsigned dc[2][16], ac[2][256];
    unsigned char zigzag[64];
    unsigned char header[JE_SCAN_OFFSET + 1];
};
constexpr int JE_DQT = 25, JE_DQT_STEP = 69, JE_SOF_SIZE = 163;   // header offsets: the luminance table's 64 bytes (chrominance: + 69); H, W (2 + 2 bytes)

constexpr JeTables je_make_tables() {
    JeTables t{};
    for (int s = 0; s < 4; ++s) {
        unsigned code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < JE_SPEC[s].bits[len - 1]; ++i, ++k, ++code) {
                const unsigned e = ((unsigned)len << 16) | code;
                if (s & 1) t.ac[s >> 1][JE_SPEC[s].vals[k]] = e;
                else t.dc[s >> 1][JE_SPEC[s].vals[k]] = e;
            }
            code <<= 1;
        }
    }
    for (int k = 0; k < 64; ++k) t.zigzag[k] = (unsigned char)je_zigzag(k);
    int n = 0;
    auto put = [&](int v) { t.header[n++] = (unsigned char)v; };
    auto seg = [&](int marker, int payload) { put(0xFF); put(marker); put((payload + 2) >> 8); put((payload + 2) & 255); };
    put(0xFF); put(0xD8);                                                     // SOI
    seg(0xE0, 14);                                                            // APP0: JFIF 1.01, no units, density 1 x 1, no thumbnail
    for (int v : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) put(v);   // "JFIF\0"
    for (int c = 0; c < 2; ++c) {                                             // DQT: 8-bit, table c, 64 entries in zigzag order
        seg(0xDB, 65);
        put(c);
        n += 64;
    }
    seg(0xC0, 15);                                                            // SOF0: 8 bits, H, W, Y 2 x 2 table 0, Cb and Cr 1 x 1 table 1
    for (int v : {8, 0, 0, 0, 0, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1}) put(v);
    for (int s = 0; s < 4; ++s) {                                             // DHT: class (s & 1), table (s >> 1)
        seg(0xC4, 17 + JE_SPEC[s].n);
        put(((s & 1) << 4) | (s >> 1));
        for (int i = 0; i < 16; ++i) put(JE_SPEC[s].bits[i]);
        for (int i = 0; i < JE_SPEC[s].n; ++i) put(JE_SPEC[s].vals[i]);
    }
    seg(0xDA, 10);                                                            // SOS: one interleaved scan of the three components, Ss 0, Se 63
    for (int v : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) put(v);
    t.header[JE_SCAN_OFFSET] = (unsigned char)(n == JE_SCAN_OFFSET);          // (checked below)
    return t;
}
constexpr JeTables JE_TABLES_HOST = je_make_tables();
static_assert(JE_TABLES_HOST.header[JE_SCAN_OFFSET] == 1, "the header is 623 bytes");
static_assert(JE_TABLES_HOST.header[JE_DQT - 5] == 0xFF && JE_TABLES_HOST.header[JE_DQT - 4] == 0xDB && JE_TABLES_HOST.header[JE_DQT + JE_DQT_STEP - 1] == 1 &&
                  JE_TABLES_HOST.header[JE_SOF_SIZE - 2] == 17 && JE_TABLES_HOST.header[JE_SOF_SIZE - 1] == 8,
              "the offsets je_write patches");
static __constant__ JeTables JE_TABLES = JE_TABLES_HOST;

// The longest block: the longest DC code with its extra bits, then 63 coefficients of the longest AC code with its extra bits (and so no EOB).
// je_walk clamps the categories to 11 (DC) and 10 (AC), what 8-bit samples can reach, so NO input makes a block longer.
constexpr int je_longest(int ac) {
    int m = 0;
    for (int t = 0; t < 2; ++t)
        for (int s = 0; s < (ac ? 256 : 12); ++s) {
            const unsigned e = ac ? JE_TABLES_HOST.ac[t][s] : JE_TABLES_HOST.dc[t][s];
            if (e && (int)(e >> 16) + (s & 15) > m) m = (int)(e >> 16) + (s & 15);
        }
    return m;
}
constexpr int JE_MAX_BLOCK_BITS = je_longest(0) + 63 * je_longest(1);
static_assert(je_longest(0) == 22 && je_longest(1) == 26 && JE_MAX_BLOCK_BITS == 1660, "Annex K: 11 + 11 bits, 16 + 10 bits");

// ---- geometry and workspace ---------------------------------------------------------------------------------------------------------
struct JeGeom {
    int H, W, mcus_x, mcus_y, rows8, cols8;   // rows8 x cols8: the Y blocks libjpeg transforms
    int nblk;                                 // blocks of an image, dummies included
    int raw_words;                            // 32-bit words of an image's raw (unstuffed) scan, a multiple of 16
    int ne;                                   // elements of JE_ELEM raw bytes
};
struct JeWork { size_t coef, bits, bsums, totbits, raw, cnt, csums, totff, total; };

static inline bool je_size_ok(int H, int W) { return H >= 8 && W >= 8 && H <= 65535 && W <= 65535; }

static inline long long je_blocks(int H, int W) { return 6LL * ((H + 15) / 16) * ((W + 15) / 16); }

// bytes of the raw scan at the most: every block at JE_MAX_BLOCK_BITS
static inline long long je_raw_bytes(int H, int W) { return (je_blocks(H, W) * JE_MAX_BLOCK_BITS + 7) / 8; }

// the stuffing pass scans ceil(raw bytes / 64) elements in two levels of JE_SCAN: about 55 megapixels; the bit offsets then fit 31 bits
static inline bool je_fits(int H, int W) { return (je_raw_bytes(H, W) + JE_ELEM - 1) / JE_ELEM <= (long long)JE_SCAN * JE_SCAN; }

static inline JeGeom je_geom(int H, int W) {
    JeGeom g{};
    g.H = H; g.W = W;
    g.mcus_x = (W + 15) / 16; g.mcus_y = (H + 15) / 16;
    g.rows8 = (H + 7) / 8; g.cols8 = (W + 7) / 8;
    g.nblk = (int)je_blocks(H, W);
    g.raw_words = (int)((((je_blocks(H, W) * JE_MAX_BLOCK_BITS + 31) / 32 + 1) + 15) / 16 * 16);
    g.ne = (int)((je_raw_bytes(H, W) + JE_ELEM - 1) / JE_ELEM);
    return g;
}

static inline size_t je_align(size_t v) { return (v + 255) & ~(size_t)255; }

static inline JeWork je_work(const JeGeom& g, int B) {
    JeWork w{};
    size_t o = 0;
    const auto take = [&](size_t bytes) { const size_t at = o; o += je_align(bytes); return at; };
    w.coef = take((size_t)B * g.nblk * 128);
    w.bits = take((size_t)B * g.nblk * 4);
    w.bsums = take((size_t)B * ((g.nblk + JE_SCAN - 1) / JE_SCAN) * 4);
    w.totbits = take((size_t)B * 4);
    w.raw = take((size_t)B * g.raw_words * 4);
    w.cnt = take((size_t)B * g.ne * 4);
    w.csums = take((size_t)B * ((g.ne + JE_SCAN - 1) / JE_SCAN) * 4);
    w.totff = take((size_t)B * 4);
    w.total = o;
    return w;
}

// ---- 1. transform -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JE_THREADS) void je_transform_kernel(const unsigned char* __restrict__ in, uint4* __restrict__ coef, JcQuality qual, JeGeom g,
                                                                  int tiles_x, int tiles_y, int total) {
    __shared__ __align__(16) unsigned char Yp[JE_YH * JE_YP];
    __shared__ __align__(16) unsigned char Cp[2][JE_CH * JE_CW];
    __shared__ int tab[2][64];
    __shared__ float rcp[2][64];
    const int tid = threadIdx.x;
    const int H = g.H, W = g.W;
    for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int tx = tile % tiles_x, tq = tile / tiles_x;
        const int ty = tq % tiles_y, img = tq / tiles_y;
        const int mx0 = tx * JE_TX, my0 = ty * JE_TY;        // the tile's first MCU
        const unsigned char* inp = in + (size_t)img * H * W * 3;
        jc_stage_tables(qual.q[img], tid, tab, rcp);
        const auto px = [&](long long o, int& r, int& gg, int& b) { const unsigned char* p = inp + 3 * o; r = p[0]; gg = p[1]; b = p[2]; };
        for (int i = tid; i < JE_CH * JE_CW; i += JE_THREADS) {
            const int qy = i / JE_CW, qx = i - qy * JE_CW;
            if (my0 + (qy >> 3) >= g.mcus_y || mx0 + (qx >> 3) >= g.mcus_x) continue;   // (no such MCU: its samples are never read)
            const JcQuad qd = jc_quad(px, my0 * 8 + qy, mx0 * 8 + qx, H, W);
            Cp[0][i] = (unsigned char)qd.cb;
            Cp[1][i] = (unsigned char)qd.cr;
            jc_quad_store_y(qd, Yp + qy * 2 * JE_YP + qx * 2, JE_YP);
        }
        __syncthreads();
        // a thread per block; `pos` is its place in the MCU's scan order
        const unsigned char* src = nullptr;
        int pitch = 0, c = 0, my = 0, mx = 0, pos = 0;
        if (tid < JE_YBLOCKS) {
            const int by = tid / (2 * JE_TX), bx = tid - by * (2 * JE_TX);
            my = my0 + (by >> 1); mx = mx0 + (bx >> 1); pos = (by & 1) * 2 + (bx & 1);
            if (my * 2 + (by & 1) < g.rows8 && mx * 2 + (bx & 1) < g.cols8) { src = Yp + by * 8 * JE_YP + bx * 8; pitch = JE_YP; }   // (else: a dummy)
        } else if (tid < JE_YBLOCKS + 2 * JE_CBLOCKS) {
            c = 1;
            const int ch = (tid - JE_YBLOCKS) / JE_CBLOCKS, r = (tid - JE_YBLOCKS) - ch * JE_CBLOCKS;
            const int by = r / JE_TX, bx = r - by * JE_TX;
            my = my0 + by; mx = mx0 + bx; pos = 4 + ch;
            src = Cp[ch] + by * 8 * JE_CW + bx * 8; pitch = JE_CW;
        }
        if (src && my < g.mcus_y && mx < g.mcus_x) {
            int d[64];
            jc_forward_block(src, pitch, tab[c], rcp[c], d);
            uint4* dst = coef + ((size_t)img * g.nblk + (size_t)(my * g.mcus_x + mx) * 6 + pos) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                unsigned w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    w[k] = ((unsigned)d[je_zigzag(8 * j + 2 * k)] & 0xFFFFu) | ((unsigned)d[je_zigzag(8 * j + 2 * k + 1)] << 16);
                dst[j] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        __syncthreads();   // (the next tile of this workgroup overwrites the planes and the tables)
    }
}

// ---- 2. / 5. the entropy coder of one block -----------------------------------------------------------------------------------------
// Y block `pos` (0 .. 3) of an MCU -> the position whose DC it codes: itself where libjpeg transforms it, else - a DUMMY block (jccoefct.c
// compress_data) - that of the block before it in the MCU's order, which may be a dummy itself.  right / bottom: the MCU's second block
// column / row is real.
__device__ __forceinline__ int je_dc_source(int pos, bool right, bool bottom) {
    const int top = right ? 1 : 0;                 // Y01, or Y00 for it
    if (pos < 2) return pos ? top : 0;
    if (!bottom) return top;                       // Y10 and Y11 both repeat what Y01 codes
    return pos == 2 ? 2 : (right ? 3 : 2);
}

__device__ __forceinline__ int je_dc_at(const unsigned* __restrict__ coefw, size_t blk) { return (int)(short)(coefw[blk * 32] & 0xFFFFu); }

// block i of an image (coefw: the image's coefficient words) -> its DC difference against the previous block of its component in scan order
// (0 before the first; dummies take part like real blocks), and whether it is a dummy
__device__ __forceinline__ int je_block_dc(const unsigned* __restrict__ coefw, int i, const JeGeom& g, bool* dummy) {
    const int mcu = i / 6, pos = i - mcu * 6;
    *dummy = false;
    if (pos >= 4) return je_dc_at(coefw, i) - (mcu ? je_dc_at(coefw, i - 6) : 0);
    const int my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
    const bool right = 2 * mx + 1 < g.cols8, bottom = 2 * my + 1 < g.rows8;
    const int src = je_dc_source(pos, right, bottom);
    *dummy = src != pos;
    const int dc = je_dc_at(coefw, (size_t)mcu * 6 + src);
    if (pos) return dc - je_dc_at(coefw, (size_t)mcu * 6 + je_dc_source(pos - 1, right, bottom));
    if (!mcu) return dc;
    const int pmx = mx ? mx - 1 : g.mcus_x - 1;    // the MCU before: the last of the row above at the left edge - never in the bottom MCU row
    return dc - je_dc_at(coefw, (size_t)(mcu - 1) * 6 + je_dc_source(3, 2 * pmx + 1 < g.cols8, mx ? bottom : true));
}

// the magnitude category n of v, clamped to `most`, and the code `e` = (length << 16) | code with its n extra bits appended: v itself, or
// v + 2^n - 1 (one's complement) where v < 0
__device__ __forceinline__ void je_symbol(unsigned e, int v, int n, unsigned* code, int* len) {
    const unsigned extra = (unsigned)(v < 0 ? v + (1 << n) - 1 : v) & ((1u << n) - 1u);
    *code = ((e & 0xFFFFu) << n) | extra;
    *len = (int)(e >> 16) + n;
}

__device__ __forceinline__ int je_category(int v, int most) { return min(32 - __clz(abs(v)), most); }

// the codes of one block to put(code, length), length <= 26: `row` holds its 32 coefficient words in LDS (word 0's low half, the DC, is not
// read: `diff` is given), dc / ac are the tables of its component in LDS
template <class Put>
__device__ __forceinline__ void je_walk(const unsigned* row, int diff, bool dummy, const unsigned* dc, const unsigned* ac, Put put) {
    unsigned code;
    int len;
    const int n0 = je_category(diff, 11);
    je_symbol(dc[n0], diff, n0, &code, &len);
    put(code, len);
    int run = 0;
    if (!dummy) {
        for (int k = 1; k < 64; ++k) {
            const unsigned w = row[k >> 1];
            if (!(k & 1) && w == 0) { run += 2; ++k; continue; }
            const int v = (int)(short)((k & 1) ? (w >> 16) : (w & 0xFFFFu));
            if (v == 0) { ++run; continue; }
            for (; run > 15; run -= 16) put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));   // ZRL
            const int n = je_category(v, 10);
            je_symbol(ac[(run << 4) | n], v, n, &code, &len);
            put(code, len);
            run = 0;
        }
    } else {
        run = 63;
    }
    if (run) put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));                                        // EOB
}

// by the whole workgroup: the tables and the coefficient words of its JE_THREADS blocks from g0 into LDS; the caller's barrier follows
__device__ __forceinline__ void je_stage_blocks(const unsigned* __restrict__ coefw, long long g0, long long total, unsigned* rows, unsigned (*dc)[16],
                                                unsigned (*ac)[256]) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * 256; i += JE_THREADS) ac[i >> 8][i & 255] = JE_TABLES.ac[i >> 8][i & 255];
    if (tid < 32) dc[tid >> 4][tid & 15] = JE_TABLES.dc[tid >> 4][tid & 15];
    for (int i = tid; i < JE_THREADS * 32; i += JE_THREADS)
        if (g0 + (i >> 5) < total) rows[(i >> 5) * JE_ROW + (i & 31)] = coefw[g0 * 32 + i];
}

// EMIT = false: bits[block] = its code bits.  EMIT = true: bits holds the exclusive prefix sums; the codes go to raw at that bit offset.
template <bool EMIT>
__global__ __launch_bounds__(JE_THREADS) void je_code_kernel(const unsigned* __restrict__ coefw, unsigned* __restrict__ bits, unsigned* __restrict__ raw,
                                                             JeGeom g, long long total) {
    __shared__ unsigned rows[JE_THREADS * JE_ROW];
    __shared__ unsigned dc[2][16], ac[2][256];
    const long long g0 = (long long)blockIdx.x * JE_THREADS, gi = g0 + threadIdx.x;
    je_stage_blocks(coefw, g0, total, rows, dc, ac);
    __syncthreads();
    if (gi >= total) return;
    const int img = (int)(gi / g.nblk), i = (int)(gi - (long long)img * g.nblk);
    bool dummy;
    const int diff = je_block_dc(coefw + (size_t)img * g.nblk * 32, i, g, &dummy);
    const int t = (i % 6) >= 4 ? 1 : 0;
    const unsigned* row = rows + threadIdx.x * JE_ROW;
    if (!EMIT) {
        unsigned sum = 0;
        je_walk(row, diff, dummy, dc[t], ac[t], [&](unsigned, int len) { sum += (unsigned)len; });
        bits[gi] = sum;
    } else {
        // MSB first: `acc` holds `n` (< 32) pending bits below whatever was flushed; a full word is OR-ed into the zeroed scan - the first and the
        // last word of a block are shared with its neighbours
        unsigned* dst = raw + (size_t)img * g.raw_words;
        const unsigned off = bits[gi];
        unsigned word = off >> 5;
        int n = (int)(off & 31u);
        unsigned long long acc = 0;
        je_walk(row, diff, dummy, dc[t], ac[t], [&](unsigned code, int len) {
            acc = (acc << len) | code;
            n += len;
            if (n >= 32) {
                n -= 32;
                atomicOr(dst + word++, (unsigned)(acc >> n));
                acc &= (1ull << n) - 1ull;
            }
        });
        if (n) atomicOr(dst + word, (unsigned)(acc << (32 - n)));
    }
}

// ---- 3. / 7. prefix sums --------------------------------------------------------------------------------------------------------------
// the sum of a value over the workgroup (all threads get it); `excl`: the exclusive prefix of the thread
__device__ __forceinline__ unsigned je_block_scan(unsigned v, unsigned* excl) {
    __shared__ unsigned waves[JE_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    __syncthreads();                               // (a second call of the kernel's loop: the last one's reads are done)
    if (lane == 63) waves[wave] = incl;
    __syncthreads();
    unsigned base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < JE_THREADS / 64; ++w) {
        if (w < wave) base += waves[w];
        sum += waves[w];
    }
    *excl = base + incl - v;
    return sum;
}

// grid (chunks, B): sums[b][chunk] = the sum of the chunk's JE_SCAN elements of data[b][0 .. n)
__global__ __launch_bounds__(JE_THREADS) void je_reduce_kernel(const unsigned* __restrict__ data, int n, unsigned* __restrict__ sums) {
    const unsigned* p = data + (size_t)blockIdx.y * n;
    const int i0 = blockIdx.x * JE_SCAN + threadIdx.x * 8;
    unsigned s = 0, excl;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += i0 + j < n ? p[i0 + j] : 0u;
    const unsigned sum = je_block_scan(s, &excl);
    if (threadIdx.x == 0) sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// grid (chunks, B): data[b][0 .. n) -> its exclusive prefix sums, chunk by chunk, in place; base (or null: one chunk) holds the exclusive prefix
// sums of the chunks' sums; totals (or null) takes the sum of the single chunk
__global__ __launch_bounds__(JE_THREADS) void je_scan_kernel(unsigned* __restrict__ data, int n, const unsigned* __restrict__ base, unsigned* __restrict__ totals) {
    unsigned* p = data + (size_t)blockIdx.y * n;
    const int i0 = blockIdx.x * JE_SCAN + threadIdx.x * 8;
    unsigned v[8], s = 0, excl;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = i0 + j < n ? p[i0 + j] : 0u;
        s += v[j];
    }
    const unsigned sum = je_block_scan(s, &excl);
    if (base) excl += base[(size_t)blockIdx.y * gridDim.x + blockIdx.x];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (i0 + j < n) p[i0 + j] = excl;
        excl += v[j];
    }
    if (totals && threadIdx.x == 0) totals[blockIdx.y] = sum;
}

// data[b][0 .. n) -> exclusive prefix sums in place, totals[b] = the sum; n <= JE_SCAN^2.  One launch, or reduce + scan of the sums + scan.
static void je_scan(unsigned* data, int n, int B, unsigned* sums, unsigned* totals, hipStream_t st) {
    const int chunks = (n + JE_SCAN - 1) / JE_SCAN;
    if (chunks == 1) {
        hipLaunchKernelGGL(je_scan_kernel, dim3(1, B), dim3(JE_THREADS), 0, st, data, n, (const unsigned*)nullptr, totals);
        return;
    }
    hipLaunchKernelGGL(je_reduce_kernel, dim3(chunks, B), dim3(JE_THREADS), 0, st, (const unsigned*)data, n, sums);
    hipLaunchKernelGGL(je_scan_kernel, dim3(1, B), dim3(JE_THREADS), 0, st, sums, chunks, (const unsigned*)nullptr, totals);
    hipLaunchKernelGGL(je_scan_kernel, dim3(chunks, B), dim3(JE_THREADS), 0, st, data, n, (const unsigned*)sums, (unsigned*)nullptr);
}

// ---- 4. zero --------------------------------------------------------------------------------------------------------------------------
// grid (x, B): the words of the image's raw scan that hold its bits, up to a whole element of the stuffing pass
__global__ __launch_bounds__(JE_THREADS) void je_zero_kernel(unsigned* __restrict__ raw, const unsigned* __restrict__ totbits, int raw_words) {
    const int need = min(raw_words, (int)((((totbits[blockIdx.y] >> 5) + 1u) + 15u) & ~15u));
    uint4* p = reinterpret_cast<uint4*>(raw + (size_t)blockIdx.y * raw_words);
    for (int i = blockIdx.x * JE_THREADS + threadIdx.x; i < need / 4; i += gridDim.x * JE_THREADS) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- 6. / 8. stuffing -----------------------------------------------------------------------------------------------------------------
// byte k (0 .. 3, big-endian) of the raw word that holds raw byte i; the last byte (i = nraw - 1) has its free bits set
__device__ __forceinline__ unsigned je_raw_byte(unsigned w, int k, int i, int nraw, unsigned tot) {
    unsigned v = (w >> (24 - 8 * k)) & 255u;
    if (i == nraw - 1 && (tot & 7u)) v |= (1u << (8 - (tot & 7u))) - 1u;
    return v;
}

// grid (x, B): cnt[b][e] = the 0xFF bytes among raw bytes [64 e, 64 e + 64) of image b (0 past its last byte)
__global__ __launch_bounds__(JE_THREADS) void je_count_kernel(const unsigned* __restrict__ raw, const unsigned* __restrict__ totbits, unsigned* __restrict__ cnt,
                                                              int raw_words, int ne) {
    const int e = blockIdx.x * JE_THREADS + threadIdx.x;
    if (e >= ne) return;
    const unsigned tot = totbits[blockIdx.y];
    const int nraw = (int)((tot + 7u) >> 3);
    unsigned c = 0;
    if (e * JE_ELEM < nraw) {
        const uint4* p = reinterpret_cast<const uint4*>(raw + (size_t)blockIdx.y * raw_words) + e * 4;
        for (int j = 0; j < 4; ++j) {
            const uint4 q = p[j];
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = e * JE_ELEM + j * 16 + k;
                if (i < nraw && je_raw_byte(w[k >> 2], k & 3, i, nraw, tot) == 255u) ++c;
            }
        }
    }
    cnt[(size_t)blockIdx.y * ne + e] = c;
}

// grid (ceil(ne / 256) + 1, B).  A thread per element: its raw bytes to the file at 623 + 64 e + cnt[b][e] (the exclusive prefix sums), a 0x00
// after every 0xFF; the thread with the last raw byte adds EOI and sets nbytes[b].  The last workgroup of an image writes its header.
__global__ __launch_bounds__(JE_THREADS) void je_write_kernel(const unsigned* __restrict__ raw, const unsigned* __restrict__ totbits, const unsigned* __restrict__ cnt,
                                                              unsigned char* __restrict__ out, int* __restrict__ nbytes, JcQuality qual, JeGeom g,
                                                              size_t out_pitch) {
    const int b = blockIdx.y;
    unsigned char* o = out + (size_t)b * out_pitch;
    if (blockIdx.x == gridDim.x - 1) {
        const int q = qual.q[b];
        for (int i = threadIdx.x; i < JE_SCAN_OFFSET; i += JE_THREADS) {
            unsigned v = JE_TABLES.header[i];
            for (int c = 0; c < 2; ++c) {
                const int k = i - (JE_DQT + c * JE_DQT_STEP);
                if (k >= 0 && k < 64) v = (unsigned)jc_table_entry(q, c, JE_TABLES.zigzag[k]);
            }
            if (i >= JE_SOF_SIZE && i < JE_SOF_SIZE + 4) v = ((i < JE_SOF_SIZE + 2 ? g.H : g.W) >> (((i - JE_SOF_SIZE) & 1) ? 0 : 8)) & 255;
            o[i] = (unsigned char)v;
        }
        return;
    }
    const int e = blockIdx.x * JE_THREADS + threadIdx.x;
    const unsigned tot = totbits[b];
    const int nraw = (int)((tot + 7u) >> 3);
    if (e >= g.ne || e * JE_ELEM >= nraw) return;
    size_t at = (size_t)JE_SCAN_OFFSET + (size_t)e * JE_ELEM + cnt[(size_t)b * g.ne + e];
    const uint4* p = reinterpret_cast<const uint4*>(raw + (size_t)b * g.raw_words) + e * 4;
    for (int j = 0; j < 4; ++j) {
        const uint4 q = p[j];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = e * JE_ELEM + j * 16 + k;
            if (i < nraw) {
                const unsigned v = je_raw_byte(w[k >> 2], k & 3, i, nraw, tot);
                o[at++] = (unsigned char)v;
                if (v == 255u) o[at++] = 0;
            }
        }
    }
    if ((e + 1) * JE_ELEM >= nraw) {
        o[at] = 0xFF;
        o[at + 1] = 0xD9;
        nbytes[b] = (int)(at + 2);
    }
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
extern "C" size_t rs_jpeg_encode_bound(int H, int W) {
    if (!je_size_ok(H, W)) return 0;
    return (size_t)JE_SCAN_OFFSET + 2 * (size_t)je_raw_bytes(H, W) + 2;
}

extern "C" size_t rs_jpeg_encode_workspace(int B, int H, int W) {
    if (B < 1 || B > RS_MAX_ROWS || !je_size_ok(H, W) || !je_fits(H, W)) return 0;
    return je_work(je_geom(H, W), B).total;
}

extern "C" int rs_jpeg_encode(const void* in_u8_nhwc, void* out, int* nbytes, const int* quality, void* workspace, int B, int C, int H, int W,
                              size_t out_pitch, void* stream) {
    const std::string who = "rs_jpeg_encode: ";
    if (!in_u8_nhwc || !out || !nbytes || !quality || !workspace) return img_fail(who, "null pointer (in / out / nbytes / quality / workspace)");
    if (B < 1 || B > RS_MAX_ROWS) return img_fail(who, "B must be 1 .. RS_MAX_ROWS (the qualities travel by value)");
    if (C != 3) return img_fail(who, "C must be 3 (RGB)");
    if (H < 8 || W < 8) return img_fail(who, "H and W must be at least 8");
    if (H > 65535 || W > 65535) return img_fail(who, "H and W must be at most 65535 (the SOF0 fields)");
    if (!je_fits(H, W)) return img_fail(who, "the image is too large (the stuffing pass scans two levels of 2048: about 55 megapixels)");
    JcQuality qual{};
    for (int b = 0; b < B; ++b) {
        if (quality[b] < 1 || quality[b] > 100) return img_fail(who, "every quality must be an integer in 1 .. 100");
        qual.q[b] = quality[b];
    }
    if (out_pitch < rs_jpeg_encode_bound(H, W)) return img_fail(who, "out_pitch is below rs_jpeg_encode_bound(H, W)");
    if ((uintptr_t)workspace % 16) return img_fail(who, "workspace must be 16-byte aligned");
    const JeGeom g = je_geom(H, W);
    const JeWork w = je_work(g, B);
    const size_t in_bytes = (size_t)B * H * W * 3, out_bytes = (size_t)B * out_pitch;
    if (img_overlaps(in_u8_nhwc, in_bytes, out, out_bytes) || img_overlaps(in_u8_nhwc, in_bytes, workspace, w.total) ||
        img_overlaps(out, out_bytes, workspace, w.total) || img_overlaps(nbytes, (size_t)B * sizeof(int), out, out_bytes) ||
        img_overlaps(nbytes, (size_t)B * sizeof(int), workspace, w.total))
        return img_fail(who, "in, out, nbytes and workspace must not overlap");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    unsigned* coefw = (unsigned*)(ws + w.coef);
    unsigned* bits = (unsigned*)(ws + w.bits);
    unsigned* totbits = (unsigned*)(ws + w.totbits);
    unsigned* raw = (unsigned*)(ws + w.raw);
    unsigned* cnt = (unsigned*)(ws + w.cnt);
    const int tiles_x = (g.mcus_x + JE_TX - 1) / JE_TX, tiles_y = (g.mcus_y + JE_TY - 1) / JE_TY;
    const int tiles = B * tiles_x * tiles_y;
    const long long blocks = (long long)B * g.nblk;
    const unsigned code_grid = (unsigned)((blocks + JE_THREADS - 1) / JE_THREADS);
    const unsigned elem_grid = (unsigned)((g.ne + JE_THREADS - 1) / JE_THREADS);
    hipLaunchKernelGGL(je_transform_kernel, dim3((unsigned)std::min(tiles, 1 << 20)), dim3(JE_THREADS), 0, st, (const unsigned char*)in_u8_nhwc, (uint4*)coefw,
                       qual, g, tiles_x, tiles_y, tiles);
    hipLaunchKernelGGL(je_code_kernel<false>, dim3(code_grid), dim3(JE_THREADS), 0, st, (const unsigned*)coefw, bits, (unsigned*)nullptr, g, blocks);
    je_scan(bits, g.nblk, B, (unsigned*)(ws + w.bsums), totbits, st);
    hipLaunchKernelGGL(je_zero_kernel, dim3((unsigned)std::min(g.raw_words / 4 / JE_THREADS + 1, 4096), B), dim3(JE_THREADS), 0, st, raw, (const unsigned*)totbits,
                       g.raw_words);
    hipLaunchKernelGGL(je_code_kernel<true>, dim3(code_grid), dim3(JE_THREADS), 0, st, (const unsigned*)coefw, bits, raw, g, blocks);
    hipLaunchKernelGGL(je_count_kernel, dim3(elem_grid, B), dim3(JE_THREADS), 0, st, (const unsigned*)raw, (const unsigned*)totbits, cnt, g.raw_words, g.ne);
    je_scan(cnt, g.ne, B, (unsigned*)(ws + w.csums), (unsigned*)(ws + w.totff), st);
    hipLaunchKernelGGL(je_write_kernel, dim3(elem_grid + 1, B), dim3(JE_THREADS), 0, st, (const unsigned*)raw, (const unsigned*)totbits, (const unsigned*)cnt,
                       (unsigned char*)out, nbytes, qual, g, out_pitch);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
