"""TEST INFRASTRUCTURE - a numpy restatement of the baseline JPEG file that Pillow (libjpeg-turbo) writes with
`Image.save(format="JPEG", quality=q, subsampling=s, restart_marker_rows=1)`, written from ITU-T T.81 and libjpeg's documented
integer arithmetic (not from csrc/jpeg.h): the oracle of the device encoder's tests.  tests/test_jpeg_ref.py pins it to Pillow
byte for byte.

    encode(image uint8 [H,W,3] | [H,W,1] | [H,W], quality, subsampling) -> Encoded(data, blocks, hist, intervals)
    write_file(blocks, h, w, ...)  -> the file of given coefficient blocks and tables (tests/jpeg_decode_ref.py's `write`)

The pipeline, in libjpeg's order:
1. RGB -> YCbCr in 16-bit fixed point (jccolor.c); grey input is its own single component;
2. the full-resolution rows replicated to the right, to the component's block width;
3. chroma: the full-resolution plane replicated down to an even height (4:2:0 only), then box downsampling with the
   alternating bias (h2v2: 1,2,1,2; h2v1: 0,1,0,1; jcsample.c);
4. ONLY THEN the last (downsampled) row replicated down to the MCU height;
5. level shift, the "islow" forward DCT (jfdctint.c: CONST_BITS 13, PASS1_BITS 2, output scaled by 8), quantisation by
   rounded division of the magnitude (jcdctmgr.c);
6. luma blocks wholly outside the component's own block extent are dummy blocks: AC zero, DC that of the block before them
   in the MCU (jccoefct.c);
7. Huffman coding with the Annex K tables, one restart interval per MCU row (jchuff.c), byte stuffing; the markers in
   libjpeg's order (jcmarker.c) with the JFIF APP0 Pillow sets (1.01, unit 0, density 1x1)."""
import collections

import numpy as np

SUBSAMPLINGS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}

# Annex K.1 quantisation tables, natural order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
# Annex K.3 Huffman tables: (number of codes of each length 1..16, the symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
    0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16,
    0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94,
    0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8,
    0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
    0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
    0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92,
    0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
    0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA])

Encoded = collections.namedtuple("Encoded", "data blocks hist intervals")


def zigzag_order():
    """natural index (8 * row + column) of zig-zag position 0..63 (T.81 figure A.6)."""
    order = sorted(range(64), key=lambda n: (n // 8 + n % 8, n // 8 if (n // 8 + n % 8) % 2 else n % 8))
    return np.array(order)


ZIGZAG = zigzag_order()


def quant_table(base, quality):
    """jpeg_set_quality(quality, force_baseline=TRUE): jpeg_quality_scaling, then (base * scale + 50) / 100 in 1..255."""
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * scale + 50) // 100, 1, 255)


def huffman_codes(table):
    """T.81 annex C: symbol -> (code, length)."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def rgb_to_ycc(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    half, offset = 1 << 15, 128 << 16
    y = (19595 * r + 38470 * g + 7471 * b + half) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + offset + half - 1) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + offset + half - 1) >> 16
    return y, cb, cr


def _pad(plane, rows, cols):
    return np.pad(plane, ((0, max(0, rows - plane.shape[0])), (0, max(0, cols - plane.shape[1]))), mode="edge")


def component_plane(full, hs, vs, hmax, vmax, mcu_rows, mcu_cols):
    """The samples of one component, padded to whole MCUs, from its full-resolution plane [H,W]."""
    h, w = full.shape
    fh, fv = hmax // hs, vmax // vs                      # this component's downsampling factors
    own_w = -(-w // fh)
    wide = _pad(full, h, -(-own_w // 8) * 8 * fh)         # right edge first, at full resolution
    if fv == 2:
        wide = _pad(wide, h + (h & 1), wide.shape[1])     # an even height BEFORE downsampling
    if (fh, fv) == (1, 1):
        small = wide
    else:
        cols = wide.shape[1] // 2
        if fv == 2:
            bias = np.tile([1, 2], cols)[:cols]
            small = (wide[0::2, 0::2] + wide[0::2, 1::2] + wide[1::2, 0::2] + wide[1::2, 1::2] + bias) >> 2
        else:
            bias = np.tile([0, 1], cols)[:cols]
            small = (wide[:, 0::2] + wide[:, 1::2] + bias) >> 1
    return _pad(small, mcu_rows * 8 * vs, mcu_cols * 8 * hs)  # downsampled rows replicated down last


def fdct_islow(blocks):
    """jfdctint.c on int64 [N,8,8] level-shifted samples -> [N,8,8] coefficients scaled by 8."""
    c = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137,
             f1_961=16069, f2_053=16819, f2_562=20995, f3_072=25172)

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    def one_pass(d, first):
        t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
        t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        out = [None] * 8
        shift = 13 - 2 if first else 13 + 2
        out[0] = (t10 + t11) << 2 if first else descale(t10 + t11, 2)
        out[4] = (t10 - t11) << 2 if first else descale(t10 - t11, 2)
        z1 = (t12 + t13) * c["f0_541"]
        out[2] = descale(z1 + t13 * c["f0_765"], shift)
        out[6] = descale(z1 - t12 * c["f1_847"], shift)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * c["f1_175"]
        t4, t5, t6, t7 = t4 * c["f0_298"], t5 * c["f2_053"], t6 * c["f3_072"], t7 * c["f1_501"]
        z1, z2 = -z1 * c["f0_899"], -z2 * c["f2_562"]
        z3, z4 = -z3 * c["f1_961"] + z5, -z4 * c["f0_390"] + z5
        out[7] = descale(t4 + z1 + z3, shift)
        out[5] = descale(t5 + z2 + z4, shift)
        out[3] = descale(t6 + z2 + z3, shift)
        out[1] = descale(t7 + z1 + z4, shift)
        return np.stack(out, -1)

    rows = one_pass([blocks[:, :, k] for k in range(8)], True)            # along each row: [N, row, frequency]
    cols = one_pass([rows[:, k, :] for k in range(8)], False)             # down each column: [N, column freq., row freq.]
    return cols.transpose(0, 2, 1)


def quantise(coefs, table):
    """(|c| + (8q >> 1)) / (8q), the sign restored."""
    q8 = (table * 8).reshape(1, 8, 8)
    mag = (np.abs(coefs) + (q8 >> 1)) // q8
    return np.where(coefs < 0, -mag, mag)


def component_blocks(plane, table):
    """-> quantised coefficients [block rows, block columns, 64] in zig-zag order."""
    rows, cols = plane.shape[0] // 8, plane.shape[1] // 8
    blocks = plane.reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8).astype(np.int64) - 128
    q = quantise(fdct_islow(blocks), table).reshape(-1, 64)[:, ZIGZAG]
    return q.reshape(rows, cols, 64)


class _Bits:
    def __init__(self, hist):
        self.out, self.acc, self.n, self.hist = bytearray(), 0, 0, hist

    def put(self, value, nbits):
        self.acc = self.acc << nbits | (value & ((1 << nbits) - 1))
        self.n += nbits
        while self.n >= 8:
            byte = self.acc >> (self.n - 8) & 255
            self._byte(byte)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def _byte(self, byte):
        self.out.append(byte)
        if byte == 255:
            self.out.append(0)
            self.hist["stuffed"] += 1

    def flush(self):
        if self.n:
            byte = (self.acc << (8 - self.n) | ((1 << (8 - self.n)) - 1)) & 255
            if byte == 255:
                self.hist["pad_ff"] += 1
            self._byte(byte)
        self.acc = self.n = 0


def _size(v):
    return int(abs(int(v))).bit_length()


def encode_block(bw, block, pred, dc_codes, ac_codes, hist):
    diff = int(block[0]) - pred
    s = _size(diff)
    hist[f"dc{s}"] += 1
    bw.put(*dc_codes[s])
    if s:
        bw.put(diff if diff >= 0 else diff - 1, s)
    run, zrl = 0, 0
    for k in range(1, 64):
        v = int(block[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac_codes[0xF0])
            hist["zrl"] += 1
            zrl += 1
            run -= 16
        s = _size(v)
        hist[f"ac{s}"] += 1
        bw.put(*ac_codes[run << 4 | s])
        bw.put(v if v >= 0 else v - 1, s)
        run = 0
    if run:
        bw.put(*ac_codes[0])
        hist["eob"] += 1
        if zrl:
            hist["zrl_then_eob"] += 1
    else:
        hist["coef63"] += 1
    return int(block[0])


def segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def encode(image, quality=75, subsampling=2):
    """-> Encoded: data (the file), blocks (per component the quantised coefficients [block rows, block columns, 64] in
    zig-zag order, dummy blocks included), hist (Counter of coded symbols: dc<size>, ac<size>, zrl, eob, coef63 - a block
    without EOB -, zrl_then_eob, stuffed, pad_ff - an interval whose padded last byte is FF) and intervals (the entropy-coded
    bytes of every restart interval)."""
    image = np.asarray(image)
    if image.ndim == 2:
        image = image[:, :, None]
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] in (1, 3), (image.dtype, image.shape)
    h, w, c = image.shape
    assert 1 <= h <= 65535 and 1 <= w <= 65535
    if c == 1:
        planes, samp, tabs = [image[:, :, 0].astype(np.int64)], [(1, 1)], [0]
    else:
        planes = list(rgb_to_ycc(image))
        samp, tabs = [{0: (1, 1), 1: (2, 1), 2: (2, 2)}[subsampling], (1, 1), (1, 1)], [0, 1, 1]
    hmax, vmax = samp[0]
    mcu_rows, mcu_cols = -(-h // (8 * vmax)), -(-w // (8 * hmax))
    qt = [quant_table(Q_LUMA, quality), quant_table(Q_CHROMA, quality)]
    blocks = []
    for plane, (hs, vs), t in zip(planes, samp, tabs):
        q = component_blocks(component_plane(plane, hs, vs, hmax, vmax, mcu_rows, mcu_cols), qt[t].reshape(8, 8))
        blocks.append(q)
    # dummy blocks: luma blocks outside the component's own extent
    own_rows, own_cols = -(-h // 8), -(-w // 8)
    luma = blocks[0]
    for my in range(mcu_rows):
        for mx in range(mcu_cols):
            prev = None
            for by in range(vmax):
                for bx in range(hmax):
                    y, x = my * vmax + by, mx * hmax + bx
                    if y >= own_rows or x >= own_cols:
                        luma[y, x, 1:] = 0
                        luma[y, x, 0] = prev
                    prev = luma[y, x, 0]

    data, hist, intervals = write_file(blocks, h, w, samp=samp, qtables=qt[:len(set(tabs))], tq=tabs, tabs=tabs,
                                       dc_tables=(DC_LUMA, DC_CHROMA), ac_tables=(AC_LUMA, AC_CHROMA), ri=mcu_cols)
    return Encoded(data, blocks, hist, intervals)


def write_file(blocks, h, w, samp, qtables, tq, tabs, dc_tables, ac_tables, ri=0, sof=0xC0, comment=b""):
    """A baseline file from quantised blocks, the markers in libjpeg's order (jcmarker.c) with the JFIF APP0 Pillow sets.
    blocks: per component int [block rows, block columns, 64] in zig-zag order, whole MCUs; samp: per component (hs, vs), the
    first the largest; qtables: the quantisation tables to define, 64 steps in natural order each, table t as number t; tq /
    tabs: per component the number of its quantisation table / of its Huffman tables; dc_tables / ac_tables: (luma, chroma)
    as (bits, symbols); ri: MCUs per restart interval, 0 for none (and no DRI); sof: the frame marker; comment: a COM
    segment.  -> (the file, Counter of coded symbols, the entropy-coded bytes of every restart interval)."""
    nc = len(blocks)
    hmax, vmax = samp[0]
    mcu_rows, mcu_cols = -(-h // (8 * vmax)), -(-w // (8 * hmax))
    for b, (hs, vs) in zip(blocks, samp):
        assert b.shape == (mcu_rows * vs, mcu_cols * hs, 64), (b.shape, mcu_rows, mcu_cols)
    hist = collections.Counter()
    dc = [huffman_codes(t) for t in dc_tables]
    ac = [huffman_codes(t) for t in ac_tables]
    total = mcu_rows * mcu_cols
    per = ri if ri else total
    intervals = []
    for i in range(-(-total // per)):
        bw = _Bits(hist)
        pred = [0] * nc
        for m in range(i * per, min(total, (i + 1) * per)):
            my, mx = divmod(m, mcu_cols)
            for ci, ((hs, vs), t) in enumerate(zip(samp, tabs)):
                for by in range(vs):
                    for bx in range(hs):
                        pred[ci] = encode_block(bw, blocks[ci][my * vs + by, mx * hs + bx], pred[ci], dc[t], ac[t], hist)
        bw.flush()
        intervals.append(bytes(bw.out))

    out = bytearray(b"\xFF\xD8")
    out += segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if comment:
        out += segment(0xFE, comment)
    for t, table in enumerate(qtables):
        out += segment(0xDB, bytes([t]) + bytes(int(v) for v in np.asarray(table)[ZIGZAG]))
    frame = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc])
    for ci, ((hs, vs), t) in enumerate(zip(samp, tq)):
        frame += bytes([ci + 1, hs << 4 | vs, t])
    out += segment(sof, frame)
    for t in range(2 if nc == 3 else 1):
        for cls, table in ((0, dc_tables[t]), (1, ac_tables[t])):
            out += segment(0xC4, bytes([cls << 4 | t]) + bytes(table[0]) + bytes(table[1]))
    if ri:
        out += segment(0xDD, ri.to_bytes(2, "big"))
    sos = bytes([nc])
    for ci, t in enumerate(tabs):
        sos += bytes([ci + 1, t << 4 | t])
    out += segment(0xDA, sos + b"\x00\x3F\x00")
    for k, data in enumerate(intervals):
        if k:
            out += bytes([0xFF, 0xD0 + (k - 1) % 8])
        out += data
    out += b"\xFF\xD9"
    return bytes(out), hist, intervals


def pil_encode(image, quality=75, subsampling=2):
    """The file Pillow writes for the same arguments."""
    import io

    import PIL.Image

    image = np.asarray(image)
    if image.ndim == 3 and image.shape[2] == 1:
        image = image[:, :, 0]
    buf = io.BytesIO()
    kw = {} if image.ndim == 2 else {"subsampling": subsampling}
    PIL.Image.fromarray(image).save(buf, format="JPEG", quality=quality, restart_marker_rows=1, **kw)
    return buf.getvalue()
