"""A baseline JPEG encoder in numpy integer arithmetic, for the tests only: the CPU restatement of excel_amd/csrc/jpeg.hip.

Written from the JPEG standard (ITU-T T.81: the marker syntax of Annex B, the example tables of Annex K, the Huffman procedures of
Annexes C and F) and from the arithmetic libjpeg documents for its default compressor: fixed-point colour conversion at scale 2^16,
4:2:0 with the (1, 2, 1, 2 ...) rounding bias, the "islow" integer DCT with 13-bit constants, quantisation that rounds half away from
zero.  encode(rgb, quality) returns the bytes `PIL.Image.fromarray(rgb).save(f, format="JPEG", quality=quality)` writes; the header is
built here, nothing is copied from an encoder's output.

The stages are kept apart (ycc / planes / fdct / coefficients / scan / stuff / header) so that a test can look at any of them."""
import numpy as np

HEADER_BYTES = 623          # SOI .. SOS for three components and the four Annex K Huffman tables
TAIL_BYTES = 2              # EOI

# natural (row-major) index of the k-th coefficient in zig-zag order (T.81 figure A.6)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# T.81 tables K.1 / K.2, natural order
QUANT_BASE = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32])

# T.81 tables K.3 - K.6: (number of codes of each length 1..16, the symbols in code order)
DC_BITS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
DC_VALS = [list(range(12)), list(range(12))]
AC_BITS = [[0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]]
AC_VALS = [
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]]


def quant_tables(quality):
    """The two tables (natural order, int64 [2,64]) at libjpeg's quality scaling: 1..100, baseline (entries clamped to 1..255)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((QUANT_BASE * scale + 50) // 100, 1, 255)


def huffman_codes(bits, vals):
    """T.81 Annex C: {symbol: (code, length)} of a table given as counts per length and symbols in code order."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def header(H, W, quality):
    """SOI, APP0 (JFIF 1.01, no units, 1 x 1), DQT x 2, SOF0 (4:2:0), DHT x 4 (DC0 AC0 DC1 AC1), SOS."""
    def seg(marker, body):
        n = len(body) + 2
        return bytes([0xFF, marker, n >> 8, n & 255]) + bytes(body)
    qt = quant_tables(quality)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2):
        out += seg(0xDB, [t] + [int(v) for v in qt[t][ZIGZAG]])
    out += seg(0xC0, [8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for t in range(2):
        out += seg(0xC4, [t] + DC_BITS[t] + DC_VALS[t])
        out += seg(0xC4, [0x10 | t] + AC_BITS[t] + AC_VALS[t])
    out += seg(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(out) == HEADER_BYTES
    return out


def ycc(rgb):
    """uint8 [H,W,3] -> (Y, Cb, Cr) int64 [H,W], fixed point at scale 2^16"""
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    half, cofs = 1 << 15, (128 << 16) + (1 << 15) - 1
    return ((19595 * r + 38470 * g + 7471 * b + half) >> 16,
            (-11059 * r - 21709 * g + 32768 * b + cofs) >> 16,
            (32768 * r - 27439 * g - 5329 * b + cofs) >> 16)


def _pad(a, rows, cols):
    """replicate the last row / column up to [rows, cols]"""
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def planes(rgb):
    """-> (Y [16 my, 16 mx], Cb, Cr [8 my, 8 mx]) before the level shift.  The luma plane is the image with its last column and row
    replicated.  The chroma planes: columns replicated up to 16 mx and the rows up to an even count BEFORE the 2 x 2 mean (bias 1, 2,
    1, 2 ... along a row), the rows of the result replicated up to 8 my AFTER it (libjpeg pads what the downsampler wrote)."""
    H, W = rgb.shape[:2]
    my, mx = -(-H // 16), -(-W // 16)
    y, cb, cr = ycc(rgb)
    out = [_pad(y, 16 * my, 16 * mx)]
    bias = np.tile([1, 2], 4 * mx)
    for c in (cb, cr):
        c = _pad(c, H + (H & 1), 16 * mx)
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(_pad(d, 8 * my, 8 * mx))
    return out


def _fdct_pass(d, first):
    """one pass of the "islow" DCT along the last axis; d int64 [...,8]"""
    C, P = 13, 2
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n
    n = C - P if first else C + P
    o = [None] * 8
    o[0] = (t10 + t11) << P if first else descale(t10 + t11, P)
    o[4] = (t10 - t11) << P if first else descale(t10 - t11, P)
    z1 = (t12 + t13) * 4433
    o[2] = descale(z1 + t13 * 6270, n)
    o[6] = descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct(blocks):
    """int64 [...,8,8] level-shifted samples -> the DCT scaled by 8: rows first (2 extra bits kept), then columns"""
    a = _fdct_pass(blocks, True)
    return np.swapaxes(_fdct_pass(np.swapaxes(a, -1, -2), False), -1, -2)


def quantise(coef, q):
    """divide by 8 q, rounding half away from zero; coef [...,64] natural order"""
    d = 8 * q
    return np.sign(coef) * ((np.abs(coef) + (d >> 1)) // d)


def _blocks(p):
    """[8 R, 8 C] -> [R, C, 8, 8]"""
    R, C = p.shape[0] // 8, p.shape[1] // 8
    return p.reshape(R, 8, C, 8).swapaxes(1, 2)


def coefficients(rgb, quality):
    """-> int64 [my * mx * 6, 64]: the quantised blocks in scan order (Y0 Y1 Y2 Y3 Cb Cr per MCU, MCUs row by row), each in zig-zag order.
    A luma block that lies wholly outside the image (right of ceil(W / 8) blocks or below ceil(H / 8)) is not transformed: it repeats the
    DC value of the block in front of it in the MCU and has no AC coefficient."""
    H, W = rgb.shape[:2]
    my, mx = -(-H // 16), -(-W // 16)
    qt = quant_tables(quality)
    y, cb, cr = planes(rgb)
    qy = quantise(fdct(_blocks(y - 128)).reshape(2 * my, 2 * mx, 64), qt[0])[..., ZIGZAG]
    qc = [quantise(fdct(_blocks(c - 128)).reshape(my, mx, 64), qt[1])[..., ZIGZAG] for c in (cb, cr)]
    out = np.zeros((my, mx, 6, 64), np.int64)
    bw, bh = -(-W // 8), -(-H // 8)
    for j in range(4):
        by, bx = np.arange(my)[:, None] * 2 + (j >> 1), np.arange(mx)[None, :] * 2 + (j & 1)
        out[:, :, j] = qy[by, bx]
        if j:
            dummy = (by >= bh) | (bx >= bw)
            out[:, :, j][dummy] = 0
            out[:, :, j, 0][dummy] = out[:, :, j - 1, 0][dummy]
    out[:, :, 4], out[:, :, 5] = qc
    return out.reshape(-1, 64)


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length

    def bytes(self):
        pad = -self.n % 8
        v = (self.acc << pad) | ((1 << pad) - 1)            # the last byte is filled with 1-bits
        return v.to_bytes((self.n + pad) // 8, "big")


def scan(coef):
    """T.81 F.1.2: the blocks of coefficients() -> the entropy-coded segment before byte stuffing"""
    dc = [huffman_codes(DC_BITS[t], DC_VALS[t]) for t in range(2)]
    ac = [huffman_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]
    bits = _Bits()
    pred = [0, 0, 0]
    for k, blk in enumerate(coef.tolist()):
        comp = (0, 0, 0, 0, 1, 2)[k % 6]
        t = min(comp, 1)
        diff, pred[comp] = blk[0] - pred[comp], blk[0]
        s = abs(diff).bit_length()
        bits.put(*dc[t][s])
        bits.put(diff if diff >= 0 else diff - 1, s)
        run = 0
        for v in blk[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                bits.put(*ac[t][0xF0])
                run -= 16
            s = abs(v).bit_length()
            bits.put(*ac[t][(run << 4) | s])
            bits.put(v if v >= 0 else v - 1, s)
            run = 0
        if run:
            bits.put(*ac[t][0x00])
    return bits.bytes()


def stuff(data):
    return data.replace(b"\xff", b"\xff\x00")


def encode(rgb, quality=75):
    """uint8 [H,W,3] -> the bytes of the JFIF file"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    H, W = rgb.shape[:2]
    return header(H, W, quality) + stuff(scan(coefficients(rgb, quality))) + b"\xff\xd9"
