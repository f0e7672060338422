// RGB images -> baseline JPEG files on the device (include/excel_hip.h, "CAM overlay JPEG files"): the imageio.imsave of
// tools/infer_lam.py:104,111 for a whole ragged batch of overlays, so that only finished file bytes cross to the host.
//
// Every stage is integer arithmetic, the one libjpeg's default compressor does, so the files are byte for byte what Pillow writes at the
// same quality: fixed-point colour conversion (scale 2^16), 4:2:0 with the 1, 2, 1, 2 rounding bias, the "islow" DCT (13-bit constants,
// 2 extra bits after the row pass, output scaled by 8), quantisation by 8 q rounding half away from zero, the Annex K Huffman tables.
// Padding as libjpeg pads: luma = the image with its last column and row replicated; chroma = columns replicated up to the MCU width and
// rows up to an even count BEFORE the 2 x 2 mean, rows of the result replicated AFTER it; a luma block that lies wholly outside the image
// is not transformed: it repeats the DC value of the block in front of it in the MCU and has no AC coefficient.
//
//   jpeg_table_kernel       32 image records per launch, passed by value (the host arrays are never read by the device)
//   jpeg_transform_kernel   one wave per 16 x 16 MCU: pixels -> LDS once, colour conversion, downsample, DCT, quantisation; the six
//                           blocks' coefficients (Y0 Y1 Y2 Y3 Cb Cr) in zig-zag order, int16, to workspace
//   jpeg_code_kernel<false> one wave per block, one lane per coefficient: the bit length of the block's Huffman code
//   jpeg_layout_kernel      one workgroup per image: scan of the block lengths (-> start bits), the 1-bits that fill the last byte
//   jpeg_code_kernel<true>  the same walk; every lane ORs its code into the cleared UNSTUFFED stream with 32-bit vector atomics (an OR
//                           is order-independent: the bytes are a pure function of the pixels and the quality)
//   jpeg_count_kernel       one workgroup per image: the 0xFF bytes of its unstuffed stream -> the size of the file
//   jpeg_offsets_kernel     one workgroup: scan of the file sizes -> (offset, size) of every file; size -1 where a file would end
//                           behind the arena
//   jpeg_assemble_kernel    one workgroup per image: header, the stream with a 0x00 behind every 0xFF, EOI
//
// The walk of a block: lane i holds coefficient i of the zig-zag order (lane 0 the DC difference to the previous block of the same
// component).  A ballot of the non-zero AC lanes gives every such lane the zero run in front of it (the distance to the previous set bit),
// so it knows its own code: run / 16 ZRL codes, the code of (run % 16, category), the amplitude bits.  Lane 63 carries the EOB when the
// last coefficient is zero.  A wave prefix sum over the lanes' bit counts places the codes.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#define JPEG_HDR 623u                  // SOI, APP0, 2 DQT, SOF0, 4 DHT, SOS
#define JPEG_TAIL 2u                   // EOI
#define JPEG_BLOCK_BYTES 208u          // bound of one block's code: 64 coefficients of at most 16 + 10 bits (DC: 9 + 11)
#define JPEG_CHUNK 64u                 // bytes of the unstuffed stream a thread copies at a time
#define JPEG_TABLE_BATCH 32

struct JpegRec {                       // one image, built by the host
    long long src;                     // byte offset of the pixels
    long long blk0;                    // first block in the coefficient / start-bit arrays
    long long word0;                   // first 32-bit word of its unstuffed stream
    int H, W, mx, my;                  // size, MCUs per row / column
};
struct JpegDyn {                       // one image, found on the device
    unsigned long long bits;           // bits of the entropy-coded segment
    long long size;                    // bytes of the file
};
struct JpegRecBatch { JpegRec r[JPEG_TABLE_BATCH]; };

// ---------------------------------------------------------------- tables (ITU-T T.81 Annex K, figure A.6), built at compile time
struct JpegTables {
    uint8_t hdr[JPEG_HDR + 1];         // the header with zero size and quantisation entries
    uint8_t zz[64];                    // natural index of the k-th zig-zag coefficient
    uint8_t qbase[2][64];              // K.1 / K.2, natural order
    unsigned dc[2][16];                // category -> code << 5 | length
    unsigned ac[2][256];               // run << 4 | category -> code << 5 | length
    unsigned hdr_len;
};
#define JPEG_OFF_DQT0 25
#define JPEG_OFF_DQT1 94
#define JPEG_OFF_SIZE 163

constexpr uint8_t JPEG_ZZ[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t JPEG_QBASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr uint8_t JPEG_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t JPEG_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t JPEG_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

struct JpegHdrWriter {
    JpegTables& t;
    unsigned n;
    constexpr void put(unsigned v) { t.hdr[n < JPEG_HDR ? n : JPEG_HDR] = (uint8_t)v, ++n; }
    constexpr void seg(unsigned marker, unsigned body) { put(0xFF), put(marker), put((body + 2) >> 8), put((body + 2) & 255); }
};

constexpr JpegTables jpeg_make_tables() {
    JpegTables t{};
    for (int i = 0; i < 64; ++i) t.zz[i] = JPEG_ZZ[i], t.qbase[0][i] = JPEG_QBASE[0][i], t.qbase[1][i] = JPEG_QBASE[1][i];
    for (int k = 0; k < 2; ++k) {                              // T.81 Annex C: codes in order of length, then of appearance
        unsigned code = 0, at = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int j = 0; j < JPEG_DC_BITS[k][len - 1]; ++j) t.dc[k][at++] = (code++ << 5) | len;
            code <<= 1;
        }
        code = 0, at = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int j = 0; j < JPEG_AC_BITS[k][len - 1]; ++j) t.ac[k][JPEG_AC_VALS[k][at++]] = (code++ << 5) | len;
            code <<= 1;
        }
    }
    JpegHdrWriter w{t, 0};
    w.put(0xFF), w.put(0xD8);
    w.seg(0xE0, 14);                                           // JFIF 1.01, no units, 1 x 1, no thumbnail
    w.put('J'), w.put('F'), w.put('I'), w.put('F'), w.put(0), w.put(1), w.put(1), w.put(0), w.put(0), w.put(1), w.put(0), w.put(1), w.put(0), w.put(0);
    for (int k = 0; k < 2; ++k) {
        w.seg(0xDB, 65), w.put(k);
        for (int i = 0; i < 64; ++i) w.put(0);                 // JPEG_OFF_DQT0 / JPEG_OFF_DQT1
    }
    w.seg(0xC0, 15), w.put(8);
    w.put(0), w.put(0), w.put(0), w.put(0);                    // JPEG_OFF_SIZE: H, W
    w.put(3), w.put(1), w.put(0x22), w.put(0), w.put(2), w.put(0x11), w.put(1), w.put(3), w.put(0x11), w.put(1);
    for (int k = 0; k < 2; ++k) {
        w.seg(0xC4, 29), w.put(k);
        for (int i = 0; i < 16; ++i) w.put(JPEG_DC_BITS[k][i]);
        for (int i = 0; i < 12; ++i) w.put(i);
        w.seg(0xC4, 179), w.put(0x10 | k);
        for (int i = 0; i < 16; ++i) w.put(JPEG_AC_BITS[k][i]);
        for (int i = 0; i < 162; ++i) w.put(JPEG_AC_VALS[k][i]);
    }
    w.seg(0xDA, 10);
    w.put(3), w.put(1), w.put(0x00), w.put(2), w.put(0x11), w.put(3), w.put(0x11), w.put(0), w.put(63), w.put(0);
    t.hdr_len = w.n;
    return t;
}
static_assert(jpeg_make_tables().hdr_len == JPEG_HDR, "the header must be 623 bytes");
__constant__ JpegTables jpeg_tab = jpeg_make_tables();

// libjpeg's quality scaling, baseline: 1..100 -> percentage, entries clamped to 1..255
__host__ __device__ static inline unsigned jpeg_quant(unsigned base, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = ((int)base * scale + 50) / 100;
    return (unsigned)(v < 1 ? 1 : v > 255 ? 255 : v);
}

__global__ void jpeg_table_kernel(JpegRecBatch batch, int first, int n, JpegRec* __restrict__ recs) {
    const int i = threadIdx.x;
    if (i < JPEG_TABLE_BATCH && first + i < n) recs[first + i] = batch.r[i];
}

// ---------------------------------------------------------------- transform
// one pass of the "islow" forward DCT over 8 values in registers
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    constexpr int C = 13, P = 2, N = FIRST ? C - P : C + P;
    int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d0 = FIRST ? (t10 + t11) << P : (t10 + t11 + (1 << (P - 1))) >> P;
    d4 = FIRST ? (t10 - t11) << P : (t10 - t11 + (1 << (P - 1))) >> P;
    int z1 = (t12 + t13) * 4433;
    d2 = (z1 + t13 * 6270 + (1 << (N - 1))) >> N;
    d6 = (z1 - t12 * 15137 + (1 << (N - 1))) >> N;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d7 = (t4 + z1 + z3 + (1 << (N - 1))) >> N;
    d5 = (t5 + z2 + z4 + (1 << (N - 1))) >> N;
    d3 = (t6 + z2 + z3 + (1 << (N - 1))) >> N;
    d1 = (t7 + z1 + z4 + (1 << (N - 1))) >> N;
}

__device__ __forceinline__ int jpeg_divide(int v, unsigned q) {         // by 8 q, rounding half away from zero
    const unsigned d = 8u * q, a = (unsigned)(v < 0 ? -v : v);
    const int r = (int)((a + (d >> 1)) / d);
    return v < 0 ? -r : r;
}

__global__ __launch_bounds__(256) void jpeg_transform_kernel(const uint8_t* __restrict__ rgb, const JpegRec* __restrict__ recs, int quality,
                                                             short* __restrict__ coef) {
    __shared__ unsigned tile[4][256];          // the MCU's pixels, R | G << 8 | B << 16, rows and columns clamped to the image
    __shared__ int samp[4][6][64];             // the six blocks: samples, then coefficients (natural order)
    __shared__ unsigned qd[2][64];             // the quantisation tables at this quality (natural order)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const JpegRec rec = recs[blockIdx.y];
    const int H = rec.H, W = rec.W;
    const int nm = rec.mx * rec.my;
    if (blockIdx.x * 4 >= nm) return;          // uniform over the workgroup
    const int mraw = blockIdx.x * 4 + wave;
    const bool live = mraw < nm;
    const int m = live ? mraw : nm - 1;        // a wave without an MCU repeats the last one and writes nothing
    const int my = m / rec.mx, mx = m - my * rec.mx;
    if (tid < 128) qd[tid >> 6][lane] = jpeg_quant(jpeg_tab.qbase[tid >> 6][lane], quality);
    const uint8_t* __restrict__ src = rgb + rec.src;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = lane + 64 * j;
        const int y = min(16 * my + (p >> 4), H - 1), x = min(16 * mx + (p & 15), W - 1);
        const uint8_t* px = src + 3ll * ((long long)y * W + x);
        tile[wave][p] = (unsigned)px[0] | ((unsigned)px[1] << 8) | ((unsigned)px[2] << 16);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {              // luma
        const int p = lane + 64 * j, r = p >> 4, c = p & 15;
        const unsigned v = tile[wave][p];
        const int R = v & 255, G = (v >> 8) & 255, B = (v >> 16) & 255;
        samp[wave][(r >> 3) * 2 + (c >> 3)][(r & 7) * 8 + (c & 7)] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
    }
    {                                          // chroma: the mean of 2 x 2 converted pixels, bias 1, 2, 1, 2 along the row
        const int cy = lane >> 3, cx = lane & 7;
        const int r0 = 2 * min(8 * my + cy, (H + 1) / 2 - 1) - 16 * my;      // rows below the image repeat the last chroma row
        int cb = 0, cr = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned v = tile[wave][(r0 + (k >> 1)) * 16 + 2 * cx + (k & 1)];
            const int R = v & 255, G = (v >> 8) & 255, B = (v >> 16) & 255;
            cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
        }
        const int bias = 1 + (cx & 1);
        samp[wave][4][lane] = ((cb + bias) >> 2) - 128;
        samp[wave][5][lane] = ((cr + bias) >> 2) - 128;
    }
    __syncthreads();
    if (lane < 48) {                           // rows
        int* s = &samp[wave][lane >> 3][(lane & 7) * 8];
        int d0 = s[0], d1 = s[1], d2 = s[2], d3 = s[3], d4 = s[4], d5 = s[5], d6 = s[6], d7 = s[7];
        jpeg_fdct8<true>(d0, d1, d2, d3, d4, d5, d6, d7);
        s[0] = d0, s[1] = d1, s[2] = d2, s[3] = d3, s[4] = d4, s[5] = d5, s[6] = d6, s[7] = d7;
    }
    __syncthreads();
    if (lane < 48) {                           // columns
        int* s = &samp[wave][lane >> 3][lane & 7];
        int d0 = s[0], d1 = s[8], d2 = s[16], d3 = s[24], d4 = s[32], d5 = s[40], d6 = s[48], d7 = s[56];
        jpeg_fdct8<false>(d0, d1, d2, d3, d4, d5, d6, d7);
        s[0] = d0, s[8] = d1, s[16] = d2, s[24] = d3, s[32] = d4, s[40] = d5, s[48] = d6, s[56] = d7;
    }
    __syncthreads();
    // luma blocks wholly outside the image: the DC value of the block in front, no AC
    const bool out_x = 16 * mx + 8 >= W, out_y = 16 * my + 8 >= H;
    const int f0 = jpeg_divide(samp[wave][0][0], qd[0][0]);
    const int f1 = out_x ? f0 : jpeg_divide(samp[wave][1][0], qd[0][0]);
    const int f2 = out_y ? f1 : jpeg_divide(samp[wave][2][0], qd[0][0]);
    const int nat = jpeg_tab.zz[lane];
    short* __restrict__ dst = coef + (rec.blk0 + 6ll * m) * 64 + lane;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        int v = jpeg_divide(samp[wave][j][nat], qd[j >> 2][nat]);
        const bool dummy = (j == 1 && out_x) || (j == 2 && out_y) || (j == 3 && (out_x || out_y));
        if (dummy) v = lane ? 0 : (j == 1 ? f0 : j == 2 ? f1 : f2);
        if (live) dst[64 * j] = (short)v;
    }
}

// ---------------------------------------------------------------- entropy coding
// A lane's codes -> the unstuffed stream, most significant bit first: a 64-bit window that starts on a 32-bit word, flushed word by word
// with an atomic OR (the stream is bytes: a word is stored byte-swapped)
struct JpegSink {
    unsigned* w;
    unsigned long long acc;
    int n;
    __device__ __forceinline__ JpegSink(unsigned* words, unsigned long long bit) : w(words + (bit >> 5)), acc(0), n((int)(bit & 31)) {}
    __device__ __forceinline__ void put(unsigned field, int bits) {          // 1 <= bits <= 32, n < 32
        acc |= (unsigned long long)field << (64 - n - bits);
        n += bits;
        if (n >= 32) {
            const unsigned v = (unsigned)(acc >> 32);
            if (v) atomicOr(w, __builtin_bswap32(v));
            ++w;
            acc <<= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ void flush() {
        const unsigned v = (unsigned)(acc >> 32);
        if (v) atomicOr(w, __builtin_bswap32(v));
    }
};

// start[] = the block's bit length (after the measuring pass) / its start bit in the image's stream (after the layout pass)
template <bool EMIT>
__global__ __launch_bounds__(256) void jpeg_code_kernel(const JpegRec* __restrict__ recs, const short* __restrict__ coef,
                                                        unsigned long long* __restrict__ start, unsigned* __restrict__ words) {
    const JpegRec rec = recs[blockIdx.y];
    const long long nblk = 6ll * rec.mx * rec.my;
    const long long k = 4ll * blockIdx.x + (threadIdx.x >> 6);
    if (k >= nblk) return;                               // wave-uniform
    const int lane = threadIdx.x & 63;
    const int j = (int)(k % 6), t = j >> 2;              // block of the MCU, table
    int c = coef[(rec.blk0 + k) * 64 + lane];
    if (lane == 0) {                                     // DC: the difference to the previous block of the component in scan order
        const long long prev = j >= 1 && j <= 3 ? k - 1 : j == 0 ? k - 3 : k - 6;
        if (prev >= 0) c -= coef[(rec.blk0 + prev) * 64];
    }
    const unsigned a = (unsigned)(c < 0 ? -c : c);
    const int cat = 32 - __clz(a);                       // 0 for a == 0
    const unsigned amp = (unsigned)(c < 0 ? c - 1 : c) & ((1u << cat) - 1);
    const unsigned long long nz = __ballot(lane > 0 && c != 0);
    unsigned code = 0, zrl = 0;                          // (code << 5 | length) of this lane's symbol; ZRL codes in front of it
    if (lane == 0) {
        code = jpeg_tab.dc[t][cat];
    } else if (c != 0) {
        const unsigned long long below = (nz | 1ull) & ((1ull << lane) - 1);
        const int run = lane - (63 - __clzll((long long)below)) - 1;
        zrl = run >> 4;
        code = jpeg_tab.ac[t][((run & 15) << 4) | cat];
    } else if (lane == 63) {
        code = jpeg_tab.ac[t][0];                        // EOB: the block ends in zeros
    }
    const unsigned zcode = jpeg_tab.ac[t][0xF0];
    const unsigned nb = code ? zrl * (zcode & 31) + (code & 31) + cat : 0;          // cat = 0 for the EOB lane
    unsigned inc = nb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (!EMIT) {
        if (lane == 63) start[rec.blk0 + k] = inc;
        return;
    }
    if (nb) {
        JpegSink s(words + rec.word0, start[rec.blk0 + k] + inc - nb);
        for (unsigned i = 0; i < zrl; ++i) s.put(zcode >> 5, zcode & 31);
        s.put(((code >> 5) << cat) | amp, (code & 31) + cat);                 // at most 16 + 11 bits
        s.flush();
    }
}

// inclusive scan over the 256 threads (red: 4 values of LDS); total = the sum over all
__device__ __forceinline__ unsigned long long jpeg_block_scan(unsigned long long v, unsigned long long* red, unsigned long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    __syncthreads();
    if (lane == 63) red[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) v += red[w];
    total = red[0] + red[1] + red[2] + red[3];
    return v;
}

__global__ __launch_bounds__(256) void jpeg_layout_kernel(const JpegRec* __restrict__ recs, unsigned long long* __restrict__ start,
                                                          JpegDyn* __restrict__ dyn, unsigned* __restrict__ words) {
    __shared__ unsigned long long red[4];
    const JpegRec rec = recs[blockIdx.x];
    const long long nblk = 6ll * rec.mx * rec.my;
    unsigned long long run = 0;
    for (long long k0 = 0; k0 < nblk; k0 += 256) {
        const long long k = k0 + threadIdx.x;
        const unsigned long long len = k < nblk ? start[rec.blk0 + k] : 0;
        unsigned long long total;
        const unsigned long long inc = jpeg_block_scan(len, red, total);
        if (k < nblk) start[rec.blk0 + k] = run + inc - len;
        run += total;
    }
    if (threadIdx.x == 0) {
        dyn[blockIdx.x].bits = run;
        if (run & 7) ((uint8_t*)(words + rec.word0))[run >> 3] = (uint8_t)(0xFFu >> (run & 7));      // the stream is still clear
    }
}

__device__ __forceinline__ unsigned jpeg_ff_bytes(unsigned w) {             // the 0xFF bytes of a word
    return (unsigned)((w & 0xFF) == 0xFF) + (unsigned)((w & 0xFF00) == 0xFF00) + (unsigned)((w & 0xFF0000) == 0xFF0000) + (unsigned)(w >= 0xFF000000u);
}

__global__ __launch_bounds__(256) void jpeg_count_kernel(const JpegRec* __restrict__ recs, JpegDyn* __restrict__ dyn, const unsigned* __restrict__ words) {
    __shared__ unsigned long long red[4];
    const JpegRec rec = recs[blockIdx.x];
    const unsigned long long ub = (dyn[blockIdx.x].bits + 7) >> 3, nw = (ub + 3) >> 2;      // bytes behind the stream are zero
    const unsigned* __restrict__ w = words + rec.word0;
    unsigned long long n = 0;
    for (unsigned long long i = threadIdx.x; i < nw; i += 256) n += jpeg_ff_bytes(w[i]);
    unsigned long long total;
    jpeg_block_scan(n, red, total);
    if (threadIdx.x == 0) dyn[blockIdx.x].size = (long long)(JPEG_HDR + ub + total + JPEG_TAIL);
}

__global__ __launch_bounds__(256) void jpeg_offsets_kernel(const JpegDyn* __restrict__ dyn, int n, unsigned long long arena_bytes,
                                                           long long* __restrict__ out_table) {
    __shared__ unsigned long long red[4];
    unsigned long long run = 0;
    for (int b0 = 0; b0 < n; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const unsigned long long size = b < n ? (unsigned long long)dyn[b].size : 0;
        unsigned long long total;
        const unsigned long long inc = jpeg_block_scan(size, red, total);
        if (b < n) {
            out_table[2 * b] = (long long)(run + inc - size);
            out_table[2 * b + 1] = run + inc <= arena_bytes ? (long long)size : -1;         // a file that would end behind the arena
        }
        run += total;
    }
}

__global__ __launch_bounds__(256) void jpeg_assemble_kernel(const JpegRec* __restrict__ recs, const JpegDyn* __restrict__ dyn, int quality,
                                                            const unsigned* __restrict__ words, const long long* __restrict__ out_table,
                                                            uint8_t* __restrict__ arena) {
    __shared__ unsigned long long red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long size = out_table[2 * b + 1];
    if (size < 0) return;                                // does not fit: its part of the arena stays untouched
    const JpegRec rec = recs[b];
    uint8_t* __restrict__ f = arena + out_table[2 * b];
    for (unsigned i = tid; i < JPEG_HDR; i += 256) {
        unsigned v = jpeg_tab.hdr[i];
        if (i >= JPEG_OFF_DQT0 && i < JPEG_OFF_DQT0 + 64) v = jpeg_quant(jpeg_tab.qbase[0][jpeg_tab.zz[i - JPEG_OFF_DQT0]], quality);
        else if (i >= JPEG_OFF_DQT1 && i < JPEG_OFF_DQT1 + 64) v = jpeg_quant(jpeg_tab.qbase[1][jpeg_tab.zz[i - JPEG_OFF_DQT1]], quality);
        else if (i == JPEG_OFF_SIZE) v = (unsigned)rec.H >> 8;
        else if (i == JPEG_OFF_SIZE + 1) v = (unsigned)rec.H & 255;
        else if (i == JPEG_OFF_SIZE + 2) v = (unsigned)rec.W >> 8;
        else if (i == JPEG_OFF_SIZE + 3) v = (unsigned)rec.W & 255;
        f[i] = (uint8_t)v;
    }
    if (tid < 2) f[size - 2 + tid] = tid ? 0xD9 : 0xFF;
    const unsigned long long ub = (dyn[b].bits + 7) >> 3;
    const uint4* __restrict__ w = (const uint4*)(words + rec.word0);         // 16-byte aligned, a whole number of chunks
    uint8_t* __restrict__ d = f + JPEG_HDR;
    unsigned long long run = 0;                          // 0x00 bytes inserted in front of this round's chunks
    for (unsigned long long c0 = 0; c0 * JPEG_CHUNK < ub; c0 += 256) {
        const unsigned long long at = (c0 + tid) * JPEG_CHUNK;               // first byte of this thread's chunk
        uint4 q[4];
        unsigned long long n = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            q[i] = at < ub ? w[(c0 + tid) * 4 + i] : make_uint4(0, 0, 0, 0);
            n += jpeg_ff_bytes(q[i].x) + jpeg_ff_bytes(q[i].y) + jpeg_ff_bytes(q[i].z) + jpeg_ff_bytes(q[i].w);
        }
        unsigned long long total;
        const unsigned long long inc = jpeg_block_scan(n, red, total);
        unsigned long long o = at + run + inc - n;       // where the chunk goes
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned word = e == 0 ? q[i].x : e == 1 ? q[i].y : e == 2 ? q[i].z : q[i].w;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const unsigned v = (word >> (8 * s)) & 255u;
                    if (at + 16 * i + 4 * e + s < ub) {
                        d[o++] = (uint8_t)v;
                        if (v == 255u) d[o++] = 0;
                    }
                }
            }
        }
        run += total;
    }
}

// ---------------------------------------------------------------- host
struct JpegPlan {
    unsigned long long arena, blocks, words, workspace;
    unsigned long long off_start, off_coef, off_words, off_dyn;      // byte offsets in the workspace (recs at 0)
    long long max_blocks;
};

// the sizes of a batch; false when an image is out of range
static bool jpeg_plan(const int32_t* hw, int n, JpegPlan& p) {
    p = JpegPlan{};
    if (!hw || n < 1) return false;
    for (int b = 0; b < n; ++b) {
        const long long H = hw[2 * b], W = hw[2 * b + 1];
        if (H < 1 || W < 1 || H > 65535 || W > 65535 || 3 * H * W >= (1ll << 31)) return false;
        const long long nblk = 6 * ((H + 15) / 16) * ((W + 15) / 16);
        p.arena += JPEG_HDR + JPEG_TAIL + 3ull * H * W;
        p.blocks += nblk;
        p.words += ((nblk * JPEG_BLOCK_BYTES + 8 + JPEG_CHUNK - 1) / JPEG_CHUNK) * (JPEG_CHUNK / 4);
        p.max_blocks = nblk > p.max_blocks ? nblk : p.max_blocks;
    }
    p.off_dyn = align_up((size_t)n * sizeof(JpegRec), 256);
    p.off_start = p.off_dyn + align_up((size_t)n * sizeof(JpegDyn), 256);
    p.off_coef = p.off_start + align_up(p.blocks * 8, 256);
    p.off_words = p.off_coef + align_up(p.blocks * 128, 256);
    p.workspace = p.off_words + align_up(p.words * 4, 256);
    return true;
}

extern "C" size_t excel_jpeg_rgb_arena_bytes(const int32_t* hw, int n) {
    JpegPlan p;
    return jpeg_plan(hw, n, p) ? (size_t)p.arena : 0;
}

extern "C" size_t excel_jpeg_rgb_workspace_bytes(const int32_t* hw, int n) {
    JpegPlan p;
    return jpeg_plan(hw, n, p) ? (size_t)p.workspace : 0;
}

extern "C" int excel_jpeg_encode_rgb_ragged(const uint8_t* rgb, const int64_t* off, const int32_t* hw, int n, int quality, uint8_t* arena,
                                            size_t arena_bytes, int64_t* out_table, void* workspace, size_t workspace_bytes, void* stream) {
    EXCEL_CHECK_ARG(rgb && off && hw && arena && out_table && workspace, "jpeg_encode_rgb_ragged: null argument");
    EXCEL_CHECK_ARG(n >= 1 && n <= 65535, "jpeg_encode_rgb_ragged: need 1 <= n <= 65535, got %d", n);
    EXCEL_CHECK_ARG(quality >= 1 && quality <= 100, "jpeg_encode_rgb_ragged: quality must be in 1..100, got %d", quality);
    EXCEL_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out_table & 7) == 0,
                    "jpeg_encode_rgb_ragged: workspace must be 16-byte aligned, out_table 8-byte aligned");
    for (int b = 0; b < n; ++b) {
        const long long H = hw[2 * b], W = hw[2 * b + 1];
        EXCEL_CHECK_ARG(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "jpeg_encode_rgb_ragged: image %d has size %lld x %lld, need 1..65535", b, H, W);
        EXCEL_CHECK_ARG(3 * H * W < (1ll << 31), "jpeg_encode_rgb_ragged: image %d (%lld x %lld): 3 H W must stay below 2^31", b, H, W);
        EXCEL_CHECK_ARG(off[b] >= 0, "jpeg_encode_rgb_ragged: image %d has byte offset %lld", b, (long long)off[b]);
    }
    JpegPlan p;
    jpeg_plan(hw, n, p);
    EXCEL_CHECK_ARG(p.blocks < (1ull << 31), "jpeg_encode_rgb_ragged: the batch is too large (%llu blocks)", p.blocks);
    EXCEL_CHECK_ARG(arena_bytes >= 1, "jpeg_encode_rgb_ragged: empty arena");
    EXCEL_CHECK_ARG(workspace_bytes >= p.workspace, "jpeg_encode_rgb_ragged: workspace of %zu bytes, need %llu (excel_jpeg_rgb_workspace_bytes)",
                    workspace_bytes, p.workspace);
    hipStream_t st = ST(stream);
    char* ws = (char*)workspace;
    JpegRec* recs = (JpegRec*)ws;
    JpegDyn* dyn = (JpegDyn*)(ws + p.off_dyn);
    unsigned long long* start = (unsigned long long*)(ws + p.off_start);
    short* coef = (short*)(ws + p.off_coef);
    unsigned* words = (unsigned*)(ws + p.off_words);
    if (hipMemsetAsync(words, 0, p.words * 4, st) != hipSuccess) {          // the codes are OR-ed in
        excel_set_error("jpeg_encode_rgb_ragged: clearing the stream failed");
        return EXCEL_ERR_LAUNCH;
    }
    long long blk0 = 0, word0 = 0;
    for (int first = 0; first < n; first += JPEG_TABLE_BATCH) {             // the records travel as kernel arguments
        JpegRecBatch batch{};
        for (int i = 0; i < JPEG_TABLE_BATCH && first + i < n; ++i) {
            const int b = first + i;
            JpegRec& r = batch.r[i];
            r.H = hw[2 * b], r.W = hw[2 * b + 1];
            r.my = (r.H + 15) / 16, r.mx = (r.W + 15) / 16;
            r.src = off[b], r.blk0 = blk0, r.word0 = word0;
            const long long nblk = 6ll * r.mx * r.my;
            blk0 += nblk;
            word0 += ((nblk * JPEG_BLOCK_BYTES + 8 + JPEG_CHUNK - 1) / JPEG_CHUNK) * (JPEG_CHUNK / 4);
        }
        hipLaunchKernelGGL(jpeg_table_kernel, dim3(1), dim3(64), 0, st, batch, first, n, recs);
        EXCEL_CHECK_LAUNCH("jpeg_table");
    }
    const long long max_mcu = p.max_blocks / 6;
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)cdivl(max_mcu, 4), n), dim3(256), 0, st, rgb, (const JpegRec*)recs, quality, coef);
    EXCEL_CHECK_LAUNCH("jpeg_transform");
    const dim3 cgrid((unsigned)cdivl(p.max_blocks, 4), n);
    hipLaunchKernelGGL(jpeg_code_kernel<false>, cgrid, dim3(256), 0, st, (const JpegRec*)recs, (const short*)coef, start, (unsigned*)nullptr);
    EXCEL_CHECK_LAUNCH("jpeg_code (measure)");
    hipLaunchKernelGGL(jpeg_layout_kernel, dim3(n), dim3(256), 0, st, (const JpegRec*)recs, start, dyn, words);
    EXCEL_CHECK_LAUNCH("jpeg_layout");
    hipLaunchKernelGGL(jpeg_code_kernel<true>, cgrid, dim3(256), 0, st, (const JpegRec*)recs, (const short*)coef, start, words);
    EXCEL_CHECK_LAUNCH("jpeg_code (emit)");
    hipLaunchKernelGGL(jpeg_count_kernel, dim3(n), dim3(256), 0, st, (const JpegRec*)recs, dyn, (const unsigned*)words);
    EXCEL_CHECK_LAUNCH("jpeg_count");
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(256), 0, st, (const JpegDyn*)dyn, n, (unsigned long long)arena_bytes, (long long*)out_table);
    EXCEL_CHECK_LAUNCH("jpeg_offsets");
    hipLaunchKernelGGL(jpeg_assemble_kernel, dim3(n), dim3(256), 0, st, (const JpegRec*)recs, (const JpegDyn*)dyn, quality, (const unsigned*)words,
                       (const long long*)out_table, arena);
    EXCEL_CHECK_LAUNCH("jpeg_assemble");
    return EXCEL_OK;
}
