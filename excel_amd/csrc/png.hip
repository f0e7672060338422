// Label maps -> palette PNG files on the device (include/excel_hip.h, "label PNG files"): the imsave of tools/infer_lam.py:95 /
// tools/training_free_attr.py:225 for a whole ragged batch, so that only finished file bytes cross to the host.
//
// A label map is long runs of one byte.  The deflate stream is ONE block with the fixed Huffman table (BTYPE = 01) that holds literals and
// matches at distance 1 only (run-length coding: zlib's Z_RLE + Z_FIXED): no tree, no match search, and every scanline (filter type 0:
// the byte 0, then the W label bytes) is coded independently of the others.  A run of L equal bytes is
//     literal, (L - 1) / 258 matches of 258, then the remainder r = (L - 1) % 258: one match of r if r >= 3, else r literals.
// Rows are joined at BIT granularity: a scan over the rows' bit lengths gives every row its start bit, and the lanes OR their codes into
// the zeroed arena with 32-bit vector atomics (an OR is order-independent: the bytes are a pure function of the labels and the palette).
//
//   png_rows_kernel<false>   one wave per scanline: bit length of the row + its two Adler-32 sums          -> row records
//   png_layout_kernel        one workgroup per image: scan of the row lengths (-> start bits), Adler-32 of the image, every byte of
//                            the file around the deflate data (signature, IHDR, PLTE, IDAT header, zlib header, Adler-32, IEND), the
//                            (offset, size) record of the image
//   png_rows_kernel<true>    one wave per scanline: the same walk, lanes that close a run emit its codes
//   png_crc_kernel           one workgroup per image: the CRC-32 of the three chunks, a slice per lane, slices combined with x^(8 n) mod P
//
// The wave walk of a scanline: 64 positions at a time, position p starts a run when symbol p differs from symbol p - 1 (position 0 and the
// position behind the last symbol always do).  The lane AT a run start closes the run in front of it: that run began at the previous set
// bit of the ballot (or at the start carried over from earlier chunks), so its length and its byte are known there, and a wave prefix sum
// over the runs' bit lengths places the codes.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#define PNG_HDR 823u           // bytes in front of the deflate data: signature 8, IHDR 25, PLTE 780, IDAT length + type 8, zlib header 2
#define PNG_TAIL 20u           // behind it: Adler-32 4, IDAT CRC 4, IEND 12
#define PNG_ALLOWANCE 880u     // PNG_HDR + PNG_TAIL + the block header / end-of-block bits, rounded up
#define PNG_ADLER 65521u
#define PNG_POLY 0xEDB88320u   // CRC-32, reflected

// bytes that bound one file: every symbol as a 9-bit literal (a match spends at most 18 bits on at least 3 symbols)
__host__ __device__ static inline unsigned long long png_bound(int H, int W) {
    const unsigned long long bits = 9ull * (unsigned long long)(W + 1) * (unsigned long long)H;
    return ((bits + 7) / 8 + PNG_ALLOWANCE + 15) & ~15ull;
}

// ---------------------------------------------------------------- fixed-Huffman codes (RFC 1951 3.2.6), packed for an LSB-first stream:
// Huffman codes go in most-significant bit first (so they are bit-reversed here), extra bits least-significant bit first
__host__ __device__ static inline int png_lit_bits(unsigned v) { return v < 144 ? 8 : 9; }
__host__ __device__ static inline unsigned png_lit_code(unsigned v) {
    return v < 144 ? __builtin_bitreverse32(0x30 + v) >> 24 : __builtin_bitreverse32(0x190 + (v - 144)) >> 23;
}
// a match of `len` (3..258) bytes at distance 1: length code, its extra bits, distance code 0 (five 0 bits) -> (field, bits)
__host__ __device__ static inline unsigned png_match_code(int len, int& nbits) {
    const unsigned l = (unsigned)(len - 3);
    const int e = len == 258 ? 0 : (l < 8 ? 0 : 29 - __builtin_clz(l));                   // extra bits of the length code
    const unsigned sym = len == 258 ? 285 : 257 + 4 * e + (l >> e);
    const int hb = sym < 280 ? 7 : 8;
    const unsigned huff = sym < 280 ? sym - 256 : 0xC0 + (sym - 280);
    const unsigned extra = len == 258 ? 0 : l & ((1u << e) - 1);
    nbits = hb + e + 5;
    return (__builtin_bitreverse32(huff) >> (32 - hb)) | (extra << hb);
}
__host__ __device__ static inline unsigned png_run_bits(unsigned v, int L) {
    const int rem = L - 1, k = rem / 258, r = rem - 258 * k, lb = png_lit_bits(v);
    int mb = 0;
    if (r >= 3) png_match_code(r, mb);
    return (unsigned)(lb + 13 * k + (r >= 3 ? mb : r * lb));
}
template <class Sink>
__host__ __device__ static inline void png_emit_run(Sink& s, unsigned v, int L) {
    const int rem = L - 1, k = rem / 258, r = rem - 258 * k, lb = png_lit_bits(v);
    const unsigned lc = png_lit_code(v);
    s.put(lc, lb);
    int mb;
    const unsigned m258 = png_match_code(258, mb);
    for (int i = 0; i < k; ++i) s.put(m258, 13);
    if (r >= 3) {
        const unsigned mc = png_match_code(r, mb);
        s.put(mc, mb);
    } else {
        for (int i = 0; i < r; ++i) s.put(lc, lb);
    }
}

// ---------------------------------------------------------------- CRC-32 over GF(2): crc(A|B) = crc(A) * x^(8 |B|) mod P  xor  crc(B)
__host__ __device__ static inline unsigned png_crc_mul(unsigned a, unsigned b) {      // a * b mod P, reflected: bit 31 = x^0
    unsigned p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1) p ^= b;
        b = (b >> 1) ^ ((b & 1) ? PNG_POLY : 0u);
    }
    return p;
}
__host__ __device__ static inline unsigned png_crc_xpow8(unsigned long long nbytes) {  // x^(8 nbytes) mod P
    unsigned r = 0x80000000u, base = 0x40000000u;
    for (unsigned long long e = 8 * nbytes; e; e >>= 1) {
        if (e & 1) r = png_crc_mul(r, base);
        base = png_crc_mul(base, base);
    }
    return r;
}
__host__ __device__ static inline unsigned png_crc_bytes(const uint8_t* p, unsigned n) {
    unsigned c = ~0u;
    for (unsigned i = 0; i < n; ++i) {
        c ^= p[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) c = (c >> 1) ^ ((c & 1) ? PNG_POLY : 0u);
    }
    return ~c;
}

// ---------------------------------------------------------------- device side
// A lane's codes -> the arena: a 64-bit window that starts on a 32-bit word of the arena, flushed word by word with an atomic OR
struct PngSink {
    unsigned* w;
    unsigned long long acc;
    int n;
    __device__ __forceinline__ PngSink(unsigned* words, unsigned long long bit) : w(words + (bit >> 5)), acc(0), n((int)(bit & 31)) {}
    __device__ __forceinline__ void put(unsigned field, int bits) {          // bits <= 18, n < 32
        acc |= (unsigned long long)field << n;
        n += bits;
        if (n >= 32) {
            if ((unsigned)acc) atomicOr(w, (unsigned)acc);
            ++w;
            acc >>= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ void flush() {
        if ((unsigned)acc) atomicOr(w, (unsigned)acc);
    }
};

// row record: x = bit length of the row (measuring pass) / its start bit in the deflate stream (after the layout pass);
// y = (sum of the row's bytes) mod 65521 | (sum of (W + 1 - j) * byte_j) mod 65521 << 16, j = index in the scanline (filter byte = 0)
template <bool EMIT>
__global__ __launch_bounds__(256) void png_rows_kernel(const uint8_t* __restrict__ labels, const int32_t* __restrict__ tab, int Hmax,
                                                       uint2* __restrict__ rows, const long long* __restrict__ out_table, unsigned* __restrict__ words) {
    const int b = blockIdx.y;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int* rec = tab + EXCEL_RAG_REC * b;
    const int H = rec[0], W = rec[1];
    if (r >= H) return;                                  // wave-uniform
    const uint8_t* __restrict__ row = labels + rec[4] + (long long)r * W;
    uint2* slot = rows + (long long)b * Hmax + r;
    const int n = W + 1;                                 // symbols of the scanline
    unsigned long long bit0 = 0;
    if (EMIT) bit0 = 8ull * ((unsigned long long)out_table[2 * b] + PNG_HDR) + slot->x;
    int carry = 0;                                       // the last run start of the earlier chunks
    unsigned base = 0;                                   // bits of the runs closed in the earlier chunks
    unsigned s1 = 0;
    unsigned long long s2 = 0;
    for (int c0 = 0; c0 <= n; c0 += 64) {
        const int p = c0 + lane;
        unsigned cur = 0, prev = 0;                      // symbols p and p - 1 (symbol 0 = the filter byte)
        if (p >= 1 && p < n) cur = row[p - 1];
        if (p >= 2 && p <= n) prev = row[p - 2];
        const bool start = p <= n && (p == 0 || p == n || cur != prev);
        const unsigned long long m = __ballot(start);
        unsigned nb = 0;
        int L = 0;
        if (start && p > 0) {                            // close the run that ends at p - 1
            const unsigned long long lower = m & ((1ull << lane) - 1);
            const int q = lower ? c0 + 63 - __clzll((long long)lower) : carry;
            L = p - q;
            nb = png_run_bits(prev, L);
        }
        unsigned inc = nb;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (EMIT && nb) {
            PngSink s(words, bit0 + base + inc - nb);
            png_emit_run(s, prev, L);
            s.flush();
        }
        base += __shfl(inc, 63, 64);
        if (m) carry = c0 + 63 - __clzll((long long)m);
        if (!EMIT) {
            s1 += cur;
            s2 += (unsigned long long)(n - p) * cur;     // cur = 0 outside 1 <= p < n
        }
    }
    if (!EMIT) {
        unsigned t2 = (unsigned)(s2 % PNG_ADLER);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s1 += __shfl_xor(s1, o, 64);
            t2 += __shfl_xor(t2, o, 64);
        }
        if (lane == 0) *slot = make_uint2(base, (s1 % PNG_ADLER) | ((t2 % PNG_ADLER) << 16));
    }
}

__device__ __forceinline__ unsigned png_be(unsigned v, int k) { return (v >> (8 * (3 - k))) & 255u; }

// sum over the 256 threads, in every thread (red: 4 words of LDS)
__device__ __forceinline__ unsigned png_block_sum(unsigned v, unsigned* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void png_layout_kernel(const int32_t* __restrict__ tab, int Hmax, const uint8_t* __restrict__ palette,
                                                         uint2* __restrict__ rows, uint8_t* __restrict__ arena, long long* __restrict__ out_table) {
    __shared__ unsigned red[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = tab[EXCEL_RAG_REC * b], W = tab[EXCEL_RAG_REC * b + 1];
    unsigned long long off = 0;                          // slots of the images in front, each of png_bound bytes (scalar loop)
    for (int i = 0; i < b; ++i) off += png_bound(tab[EXCEL_RAG_REC * i], tab[EXCEL_RAG_REC * i + 1]);
    uint2* rr = rows + (long long)b * Hmax;
    const unsigned n = (unsigned)W + 1;
    unsigned run = 3;                                    // the block header: BFINAL = 1, BTYPE = 01
    unsigned a = 0, bs = 0;
    for (int r0 = 0; r0 < H; r0 += 256) {
        const int r = r0 + tid;
        const uint2 rec = r < H ? rr[r] : make_uint2(0, 0);
        unsigned inc = rec.x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        __syncthreads();
        if (lane == 63) red[wave] = inc;
        __syncthreads();
        unsigned before = 0;
        for (int w = 0; w < wave; ++w) before += red[w];
        if (r < H) rr[r].x = run + before + inc - rec.x;
        run += red[0] + red[1] + red[2] + red[3];
        if (r < H) {
            const unsigned s1 = rec.y & 0xffffu, s2 = rec.y >> 16;
            const unsigned long long after = ((unsigned long long)(H - 1 - r) * n) % PNG_ADLER;      // bytes behind this row
            a = (a + s1) % PNG_ADLER;
            bs = (unsigned)((bs + s2 + after * s1) % PNG_ADLER);
        }
    }
    a = png_block_sum(a, red);
    bs = png_block_sum(bs, red);
    const unsigned A = (1u + a) % PNG_ADLER;
    const unsigned Bv = (unsigned)((((unsigned long long)H * n) % PNG_ADLER + bs) % PNG_ADLER);
    const unsigned adler = (Bv << 16) | A;
    const unsigned dbytes = (run + 7 + 7) >> 3;          // + the 7-bit end-of-block code (all zero: nothing to write)
    const unsigned idat = 2 + dbytes + 4;
    uint8_t* f = arena + off;
    for (unsigned i = tid; i <= PNG_HDR; i += 256) {     // the arena is zero: the CRC fields are left for png_crc_kernel
        unsigned v = 0;
        if (i < 8) v = (unsigned)(0x0A1A0A0D474E5089ull >> (8 * i)) & 255u;
        else if (i < 12) v = png_be(13, i - 8);
        else if (i < 16) v = png_be(0x49484452u, i - 12);            // IHDR
        else if (i < 20) v = png_be((unsigned)W, i - 16);
        else if (i < 24) v = png_be((unsigned)H, i - 20);
        else if (i == 24) v = 8;                                     // bit depth
        else if (i == 25) v = 3;                                     // colour type: palette
        else if (i < 33) v = 0;                                      // compression, filter, interlace; CRC
        else if (i < 37) v = png_be(768, i - 33);
        else if (i < 41) v = png_be(0x504C5445u, i - 37);            // PLTE
        else if (i < 809) v = palette[i - 41];
        else if (i < 813) v = 0;                                     // CRC
        else if (i < 817) v = png_be(idat, i - 813);
        else if (i < 821) v = png_be(0x49444154u, i - 817);          // IDAT
        else if (i == 821) v = 0x78;                                 // zlib: deflate, 32 K window
        else if (i == 822) v = 0x01;                                 // (0x7801 % 31 == 0)
        else v = 0x03;                                               // first deflate byte: the block header bits
        if (v) f[i] = (uint8_t)v;
    }
    if (tid < PNG_TAIL) {
        uint8_t* t = f + PNG_HDR + dbytes;
        unsigned v = 0;
        if (tid < 4) v = png_be(adler, tid);
        else if (tid >= 12 && tid < 16) v = png_be(0x49454E44u, tid - 12);   // IEND (length 0)
        else if (tid >= 16) v = png_be(0xAE426082u, tid - 16);               // its CRC
        if (v) t[tid] = (uint8_t)v;
    }
    if (tid == 0) {
        out_table[2 * b] = (long long)off;
        out_table[2 * b + 1] = (long long)(PNG_HDR + dbytes + PNG_TAIL);
    }
}

// CRC-32 of n bytes by the 256 threads of a workgroup: a slice per thread, slice t weighted with x^(8 * bytes behind it) mod P
__device__ __forceinline__ unsigned png_block_crc(const uint8_t* __restrict__ p, unsigned n, unsigned* red) {
    const unsigned s = (n + 255) / 256;
    const unsigned lo = min(n, threadIdx.x * s), hi = min(n, lo + s);
    unsigned c = 0;
    if (hi > lo) c = png_crc_mul(png_crc_xpow8(n - hi), png_crc_bytes(p + lo, hi - lo));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    return red[0] ^ red[1] ^ red[2] ^ red[3];
}

__global__ __launch_bounds__(256) void png_crc_kernel(uint8_t* __restrict__ arena, const long long* __restrict__ out_table) {
    __shared__ unsigned red[4];
    const int b = blockIdx.x;
    uint8_t* f = arena + out_table[2 * b];
    const unsigned dbytes = (unsigned)out_table[2 * b + 1] - PNG_HDR - PNG_TAIL;
    const unsigned c0 = png_block_crc(f + 12, 17, red);                      // IHDR: type + 13
    const unsigned c1 = png_block_crc(f + 37, 772, red);                     // PLTE: type + 768
    const unsigned c2 = png_block_crc(f + 817, 4 + 2 + dbytes + 4, red);     // IDAT: type + zlib header + deflate data + Adler-32
    if (threadIdx.x < 12) {
        const int k = threadIdx.x & 3, which = threadIdx.x >> 2;
        const unsigned c = which == 0 ? c0 : which == 1 ? c1 : c2;
        const unsigned at = which == 0 ? 29 : which == 1 ? 809 : PNG_HDR + dbytes + 4;
        f[at + k] = (uint8_t)png_be(c, k);
    }
}

extern "C" size_t excel_png_labels_bound_bytes(int H, int W) { return H >= 1 && W >= 1 ? (size_t)png_bound(H, W) : 0; }

extern "C" size_t excel_png_labels_workspace_bytes(int B, int max_h) {
    return B >= 1 && max_h >= 1 ? (size_t)B * (size_t)max_h * sizeof(uint2) : 0;
}

extern "C" int excel_png_encode_labels_ragged(const uint8_t* labels, const int32_t* table, const excel_ragged_info* info, const int32_t* hw,
                                              const uint8_t* palette, uint8_t* arena, size_t arena_bytes, int64_t* out_table, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    EXCEL_CHECK_ARG(labels && table && info && hw && palette && arena && out_table && workspace, "png_encode_labels_ragged: null argument");
    const int B = info->B;
    EXCEL_CHECK_ARG(B >= 1 && B <= 65535, "png_encode_labels_ragged: need 1 <= B <= 65535, got %d", B);
    EXCEL_CHECK_ARG(((uintptr_t)arena & 3) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out_table & 7) == 0,
                    "png_encode_labels_ragged: arena must be 4-byte aligned, workspace and out_table 8-byte aligned");
    unsigned long long need = 0, pix = 0;
    int Hmax = 0;
    for (int b = 0; b < B; ++b) {
        const int H = hw[2 * b], W = hw[2 * b + 1];
        EXCEL_CHECK_ARG(H >= 1 && W >= 1, "png_encode_labels_ragged: image %d has size %d x %d", b, H, W);
        EXCEL_CHECK_ARG(9ull * ((unsigned long long)W + 1) * (unsigned long long)H + 10 < (1ull << 32),
                        "png_encode_labels_ragged: image %d (%d x %d): 9 (W + 1) H must stay below 2^32", b, H, W);
        need += png_bound(H, W);
        pix += (unsigned long long)H * W;
        Hmax = H > Hmax ? H : Hmax;
    }
    EXCEL_CHECK_ARG(pix == (unsigned long long)info->total_label_pix, "png_encode_labels_ragged: hw holds %llu pixels, the plan %lld", pix,
                    (long long)info->total_label_pix);
    EXCEL_CHECK_ARG(arena_bytes >= need, "png_encode_labels_ragged: arena of %zu bytes, the bound of this batch is %llu (excel_png_labels_bound_bytes)",
                    arena_bytes, need);
    EXCEL_CHECK_ARG(workspace_bytes >= excel_png_labels_workspace_bytes(B, Hmax), "png_encode_labels_ragged: workspace of %zu bytes, need %zu",
                    workspace_bytes, excel_png_labels_workspace_bytes(B, Hmax));
    hipStream_t st = ST(stream);
    if (hipMemsetAsync(arena, 0, need, st) != hipSuccess) {        // the codes are OR-ed in
        excel_set_error("png_encode_labels_ragged: clearing the arena failed");
        return EXCEL_ERR_LAUNCH;
    }
    uint2* rows = (uint2*)workspace;
    const dim3 grid(cdiv(Hmax, 4), B);
    hipLaunchKernelGGL(png_rows_kernel<false>, grid, dim3(256), 0, st, labels, table, Hmax, rows, (const long long*)nullptr, (unsigned*)nullptr);
    EXCEL_CHECK_LAUNCH("png_rows (measure)");
    hipLaunchKernelGGL(png_layout_kernel, dim3(B), dim3(256), 0, st, table, Hmax, palette, rows, arena, (long long*)out_table);
    EXCEL_CHECK_LAUNCH("png_layout");
    hipLaunchKernelGGL(png_rows_kernel<true>, grid, dim3(256), 0, st, labels, table, Hmax, rows, (const long long*)out_table, (unsigned*)arena);
    EXCEL_CHECK_LAUNCH("png_rows (emit)");
    hipLaunchKernelGGL(png_crc_kernel, dim3(B), dim3(256), 0, st, arena, (const long long*)out_table);
    EXCEL_CHECK_LAUNCH("png_crc");
    return EXCEL_OK;
}
