"""Dev: a CPU walk through jpeg.hip's lane logic - the transform kernel's clamped tile, chroma rows and dummy blocks; the code kernel's
ballot / zero-run / EOB rule per lane and its 64-bit sink - against tests/_jpeg_ref.py on every case of tests/_jpeg_cases.py.
    python tools_dev/jpeg_lane_emulation.py      # prints "bad 0" """
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np, _jpeg_ref as R, _jpeg_cases as C

def tables():
    dc = [[0]*16 for _ in range(2)]; ac = [[0]*256 for _ in range(2)]
    for t in range(2):
        for s,(c,l) in R.huffman_codes(R.DC_BITS[t], R.DC_VALS[t]).items(): dc[t][s] = (c<<5)|l
        for s,(c,l) in R.huffman_codes(R.AC_BITS[t], R.AC_VALS[t]).items(): ac[t][s] = (c<<5)|l
    return dc, ac
DC, AC = tables()

def transform(rgb, q):
    H, W = rgb.shape[:2]; MY, MX = -(-H//16), -(-W//16)
    qt = R.quant_tables(q)
    out = np.zeros((MY*MX*6, 64), np.int64)
    def div(v, qq):
        d = 8*int(qq); a = abs(int(v)); r = (a + (d>>1))//d
        return -r if v < 0 else r
    for my in range(MY):
        for mx in range(MX):
            tile = np.zeros((16,16,3), np.int64)
            for r in range(16):
                for c in range(16):
                    tile[r,c] = rgb[min(16*my+r,H-1), min(16*mx+c,W-1)]
            samp = np.zeros((6,64), np.int64)
            for r in range(16):
                for c in range(16):
                    Rr,G,B = tile[r,c]
                    samp[(r>>3)*2+(c>>3)][(r&7)*8+(c&7)] = ((19595*Rr+38470*G+7471*B+32768)>>16)-128
            for lane in range(64):
                cy, cx = lane>>3, lane&7
                r0 = 2*min(8*my+cy, (H+1)//2-1) - 16*my
                assert 0 <= r0 <= 14
                cb = cr = 0
                for k in range(4):
                    Rr,G,B = tile[r0+(k>>1), 2*cx+(k&1)]
                    cb += (-11059*Rr-21709*G+32768*B+(128<<16)+32767)>>16
                    cr += (32768*Rr-27439*G-5329*B+(128<<16)+32767)>>16
                bias = 1+(cx&1)
                samp[4][lane] = ((cb+bias)>>2)-128; samp[5][lane] = ((cr+bias)>>2)-128
            co = R.fdct(samp.reshape(6,8,8)).reshape(6,64)
            out_x, out_y = 16*mx+8 >= W, 16*my+8 >= H
            f0 = div(co[0][0], qt[0][0]); f1 = f0 if out_x else div(co[1][0], qt[0][0]); f2 = f1 if out_y else div(co[2][0], qt[0][0])
            m = my*MX+mx
            for j in range(6):
                for lane in range(64):
                    nat = R.ZIGZAG[lane]
                    v = div(co[j][nat], qt[j>>2][nat])
                    dummy = (j==1 and out_x) or (j==2 and out_y) or (j==3 and (out_x or out_y))
                    if dummy: v = 0 if lane else (f0 if j==1 else f1 if j==2 else f2)
                    out[6*m+j][lane] = v
    return out

def code(coef):
    nblk = coef.shape[0]
    lens, plan = [], []
    for k in range(nblk):
        j = k % 6; t = j >> 2
        lanes = []
        c = [int(v) for v in coef[k]]
        prev = k-1 if 1 <= j <= 3 else (k-3 if j == 0 else k-6)
        if prev >= 0: c[0] -= int(coef[prev][0])
        nz = 0
        for l in range(1,64):
            if c[l] != 0: nz |= 1 << l
        for l in range(64):
            a = abs(c[l]); cat = a.bit_length()
            amp = (c[l]-1 if c[l] < 0 else c[l]) & ((1<<cat)-1)
            cd = zrl = 0
            if l == 0: cd = DC[t][cat]
            elif c[l] != 0:
                below = (nz|1) & ((1<<l)-1)
                run = l - (below.bit_length()-1) - 1
                zrl = run >> 4; cd = AC[t][((run&15)<<4)|cat]
                assert cd
            elif l == 63: cd = AC[t][0]
            z = AC[t][0xF0]
            nb = zrl*(z&31) + (cd&31) + cat if cd else 0
            lanes.append((nb, zrl, z, cd, cat, amp))
        plan.append(lanes); lens.append(sum(x[0] for x in lanes))
    starts = np.concatenate([[0], np.cumsum(lens)]); total = int(starts[-1])
    words = [0]*((total>>5)+2)
    def OR(i, v): words[i] |= int.from_bytes(v.to_bytes(4,"big"), "little")   # bswap
    class Sink:
        def __init__(s, bit): s.w = bit>>5; s.acc = 0; s.n = bit&31
        def put(s, f, bits):
            assert 1 <= bits <= 32 and s.n < 32 and f < (1<<bits)
            s.acc |= f << (64-s.n-bits); s.n += bits
            if s.n >= 32:
                v = s.acc >> 32
                if v: OR(s.w, v)
                s.w += 1; s.acc = (s.acc << 32) & (2**64-1); s.n -= 32
        def flush(s):
            v = s.acc >> 32
            if v: OR(s.w, v)
    for k, lanes in enumerate(plan):
        inc = 0
        for (nb, zrl, z, cd, cat, amp) in lanes:
            inc += nb
            if nb:
                s = Sink(int(starts[k]) + inc - nb)
                for _ in range(zrl): s.put(z>>5, z&31)
                s.put(((cd>>5)<<cat)|amp, (cd&31)+cat); s.flush()
    mem = bytearray(b"".join(w.to_bytes(4,"little") for w in words))
    if total & 7: mem[total>>3] |= 0xFF >> (total&7)
    return bytes(mem[:(total+7)>>3])

bad = 0
for s in C.SHAPES:
    for c in C.CONTENTS:
        for q in C.QUALITIES:
            a = C.image(s, c)
            ref = R.coefficients(a, q)
            co = transform(a, q)
            if not np.array_equal(co, ref): bad += 1; print("COEF", s, c, q)
            if code(co) != R.scan(ref): bad += 1; print("SCAN", s, c, q)
print("bad", bad)
