"""TEST INFRASTRUCTURE - a numpy restatement of what Pillow (libjpeg-turbo) returns for `Image.open(f).convert("RGB")` of a
baseline JPEG file, written from ITU-T T.81 and libjpeg's documented integer arithmetic (not from csrc/jpeg_decode.h): the
oracle of the device decoder's tests.  tests/test_jpeg_decode_ref.py pins it to Pillow pixel for pixel.

    parse(data)                 -> Header (the marker segments from SOI to SOS; ValueError for what the decoder refuses)
    decode(data, mode="RGB")    -> uint8 [H,W,3] ("unchanged": [H,W,1] for a grey file); ValueError for a corrupt scan
    write(planes, ...)          -> a baseline file built from given coefficient blocks and tables

The pipeline, in libjpeg's order:
1. the scan cut at its RSTm markers, `FF 00` unstuffed, each interval Huffman-decoded with the file's own tables (jdhuff.c);
   the DC predictors restart at zero in every interval;
2. dequantisation and the "islow" inverse DCT (jidctint.c: CONST_BITS 13, PASS1_BITS 2), the result + 128 saturated to
   0..255.  libjpeg's C code takes the result modulo 1024 into its range-limit table instead, which wraps for samples outside
   -512..511; the SIMD IDCT that libjpeg-turbo (and so Pillow) runs saturates, and Pillow is what this file is pinned to;
3. chroma: "fancy" (triangle) upsampling over the component's downsampled extent (jdsample.c), plain replication where the
   downsampled width is 1 or 2; the rows above the first and below the last downsampled row are copies of it (jdmainct.c);
4. YCbCr -> RGB with jdcolor.c's 16-bit fixed-point tables, cropped to H x W."""
import collections

import numpy as np

from tests import jpeg_ref as E

ZIGZAG = E.ZIGZAG
Header = collections.namedtuple("Header", "h w comps qt dc ac ri scan_start")  # comps: [(hs, vs, tq, td, ta)]
SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
             0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic coding", 0xCA: "arithmetic coding, progressive",
             0xCB: "arithmetic coding, lossless", 0xCD: "arithmetic coding", 0xCE: "arithmetic coding", 0xCF: "arithmetic coding"}


def parse(data):
    if len(data) < 4 or data[:2] != b"\xFF\xD8":
        raise ValueError("not a JPEG file: no SOI marker")
    pos, qt, dc, ac, ri, sof, adobe, jfif = 2, {}, {}, {}, 0, None, None, False
    while True:
        while pos < len(data) and data[pos] == 0xFF and pos + 1 < len(data) and data[pos + 1] == 0xFF:
            pos += 1
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise ValueError("corrupt JPEG header: no marker where one must stand")
        marker, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + n]
        if n < 2 or len(body) != n - 2:
            raise ValueError("corrupt JPEG header: a truncated segment")
        pos += 2 + n
        if marker == 0xDB:
            while body:
                if body[0] >> 4:
                    raise ValueError("unsupported JPEG: 16-bit quantisation tables")
                if len(body) < 65:
                    raise ValueError("corrupt JPEG header: a short DQT")
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = list(body[1:65])
                qt[body[0] & 15] = t
                body = body[65:]
        elif marker == 0xC4:
            while body:
                if len(body) < 17:
                    raise ValueError("corrupt JPEG header: a short DHT")
                bits = list(body[1:17])
                n_sym = sum(bits)
                if n_sym > 256 or len(body) < 17 + n_sym or (body[0] & 15) > 3 or (body[0] >> 4) > 1:
                    raise ValueError("corrupt JPEG header: a bad DHT")
                code = 0
                for length in range(1, 17):
                    code += bits[length - 1]
                    if code > (1 << length):
                        raise ValueError("corrupt JPEG header: an over-subscribed Huffman table")
                    code <<= 1
                (ac if body[0] >> 4 else dc)[body[0] & 15] = (bits, list(body[17:17 + n_sym]))
                body = body[17 + n_sym:]
        elif marker == 0xDD:
            ri = int.from_bytes(body[:2], "big")
        elif marker == 0xC0:
            if sof is not None:
                raise ValueError("corrupt JPEG header: two SOF markers")
            sof = body
        elif marker in SOF_NAMES:
            raise ValueError(f"unsupported JPEG: {SOF_NAMES[marker]} (SOF{marker - 0xC0}); baseline sequential Huffman only")
        elif marker == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif marker == 0xE0 and body[:5] == b"JFIF\x00":
            jfif = True
        elif marker == 0xDA:
            break
        elif marker == 0xD9:
            raise ValueError("corrupt JPEG: EOI before any scan")
    if sof is None or len(sof) < 6 or len(sof) != 6 + 3 * sof[5]:
        raise ValueError("corrupt JPEG header: no SOF0 before the scan")
    if sof[0] != 8:
        raise ValueError(f"unsupported JPEG: {sof[0]}-bit samples")
    h, w, nc = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    if h == 0 or w == 0:
        raise ValueError("unsupported JPEG: a zero dimension (DNL)")
    if nc not in (1, 3):
        raise ValueError(f"unsupported JPEG: {nc} components (CMYK / YCCK)" if nc == 4 else f"unsupported JPEG: {nc} components")
    ids = [sof[6 + 3 * k] for k in range(nc)]
    samp = [(sof[7 + 3 * k] >> 4, sof[7 + 3 * k] & 15) for k in range(nc)]
    tqs = [sof[8 + 3 * k] for k in range(nc)]
    if nc == 3 and (adobe == 0 or (adobe is None and not jfif and ids == [82, 71, 66])):
        raise ValueError("unsupported JPEG: an RGB file (Adobe transform 0); YCbCr only")
    if nc == 3 and adobe not in (None, 1):
        raise ValueError(f"unsupported JPEG: Adobe colour transform {adobe}")
    if nc == 1:
        samp = [(1, 1)]  # a single component is not interleaved: its sampling factors mean nothing
    elif samp[1] != (1, 1) or samp[2] != (1, 1) or samp[0] not in ((1, 1), (2, 1), (2, 2)):
        raise ValueError("unsupported JPEG: sampling factors " + ", ".join(f"{a}x{b}" for a, b in samp) + "; 4:4:4, 4:2:2 and 4:2:0 only")
    if len(body) != 4 + 2 * body[0] or body[0] != nc:
        raise ValueError("unsupported JPEG: more than one scan (a scan that does not hold every component)")
    if (body[-3], body[-2], body[-1]) != (0, 63, 0):
        raise ValueError("unsupported JPEG: a scan of part of the spectrum (progressive parameters)")
    comps = []
    for k in range(nc):
        if body[1 + 2 * k] != ids[k]:
            raise ValueError("unsupported JPEG: the scan's components are not in frame order")
        td, ta = body[2 + 2 * k] >> 4, body[2 + 2 * k] & 15
        if tqs[k] not in qt or td not in dc or ta not in ac:
            raise ValueError("corrupt JPEG header: a table the scan needs is not defined")
        comps.append((samp[k][0], samp[k][1], tqs[k], td, ta))
    return Header(h, w, comps, qt, dc, ac, ri, pos)


def intervals_of(scan):
    """The entropy-coded bytes of each restart interval, unstuffed, and the markers between them."""
    out, markers, cur, k = [], [], bytearray(), 0
    while k < len(scan):
        b = scan[k]
        if b != 0xFF:
            cur.append(b)
            k += 1
        elif k + 1 < len(scan) and scan[k + 1] == 0:
            cur.append(0xFF)
            k += 2
        else:
            m = scan[k + 1] if k + 1 < len(scan) else None
            out.append(bytes(cur))
            markers.append(m)
            cur = bytearray()
            if m is None or not 0xD0 <= m <= 0xD7:
                return out, markers
            k += 2
    out.append(bytes(cur))
    markers.append(None)
    return out, markers


class _Reader:
    def __init__(self, data):
        self.v, self.n, self.pos = int.from_bytes(data, "big") if data else 0, 8 * len(data), 0

    def peek(self, nbits):
        """the next nbits bits, zeros behind the end"""
        end = self.pos + nbits
        if end <= self.n:
            return (self.v >> (self.n - end)) & ((1 << nbits) - 1)
        return ((self.v << (end - self.n)) >> 0) & ((1 << nbits) - 1)


def decode_tables(table):
    """(code, length) -> symbol"""
    return {v: k for k, v in E.huffman_codes(table).items()}


def _symbol(rd, lookup):
    code = rd.peek(16)
    for length in range(1, 17):
        sym = lookup.get((code >> (16 - length), length))
        if sym is not None:
            rd.pos += length
            return sym
    raise ValueError("corrupt JPEG scan: a code that is not in the Huffman table")


def _value(rd, s):
    v = rd.peek(s)
    rd.pos += s
    return v if v >> (s - 1) else v - (1 << s) + 1


def decode_coefficients(data, hd=None):
    """-> per component the quantised coefficients [block rows, block columns, 64] in zig-zag order (whole MCUs)."""
    hd = hd or parse(data)
    scan = data[hd.scan_start:]
    hmax, vmax = hd.comps[0][0], hd.comps[0][1]
    mcu_rows, mcu_cols = -(-hd.h // (8 * vmax)), -(-hd.w // (8 * hmax))
    total = mcu_rows * mcu_cols
    per = hd.ri if hd.ri else total
    ivs, markers = intervals_of(scan)
    n_int = -(-total // per)
    if len(ivs) < n_int:
        raise ValueError("corrupt JPEG scan: truncated (fewer restart intervals than the header implies)")
    for k in range(n_int - 1):
        if markers[k] != 0xD0 + (k & 7):
            raise ValueError("corrupt JPEG scan: an unexpected marker")
    if markers[n_int - 1] is None:
        raise ValueError("corrupt JPEG scan: truncated (no marker ends the scan)")
    blocks = [np.zeros((mcu_rows * vs, mcu_cols * hs, 64), np.int64) for hs, vs, _, _, _ in hd.comps]
    dcl = {t: decode_tables(v) for t, v in hd.dc.items()}
    acl = {t: decode_tables(v) for t, v in hd.ac.items()}
    for i in range(n_int):
        rd = _Reader(ivs[i])
        pred = [0] * len(hd.comps)
        for m in range(i * per, min(total, (i + 1) * per)):
            my, mx = divmod(m, mcu_cols)
            for ci, (hs, vs, _, td, ta) in enumerate(hd.comps):
                for by in range(vs):
                    for bx in range(hs):
                        blk = blocks[ci][my * vs + by, mx * hs + bx]
                        s = _symbol(rd, dcl[td])
                        if s > 11:
                            raise ValueError("corrupt JPEG scan: a DC difference of more than 11 bits")
                        pred[ci] += _value(rd, s) if s else 0
                        blk[0] = pred[ci]
                        z = 1
                        while z < 64:
                            sym = _symbol(rd, acl[ta])
                            r, s = sym >> 4, sym & 15
                            if s == 0:
                                if r != 15:
                                    break
                                z += 16
                                if z > 64:
                                    raise ValueError("corrupt JPEG scan: a block of more than 64 coefficients")
                                continue
                            z += r
                            if z > 63:
                                raise ValueError("corrupt JPEG scan: a block of more than 64 coefficients")
                            blk[z] = _value(rd, s)
                            z += 1
        if rd.pos > rd.n:
            raise ValueError("corrupt JPEG scan: truncated (the interval ends inside an MCU)")
    return blocks


def idct_islow(coef):
    """jidctint.c on dequantised int64 [N,8,8] (natural order) -> samples uint8 [N,8,8]."""
    def one_pass(d, shift):
        z2, z3 = d[2], d[6]
        z1 = (z2 + z3) * 4433
        tmp2, tmp3 = z1 - z3 * 15137, z1 + z2 * 6270
        tmp0, tmp1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
        tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * 9633
        t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
        z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        out = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
        return [(o + (1 << (shift - 1))) >> shift for o in out]

    ws = np.stack(one_pass([coef[:, r, :] for r in range(8)], 11), 1)       # down each column: [N, row, column]
    out = np.stack(one_pass([ws[:, :, c] for c in range(8)], 18), 2)        # along each row
    return np.clip(out + 128, 0, 255).astype(np.uint8)                      # saturation, as libjpeg-turbo's SIMD IDCT packs


def component_plane(blocks, table):
    rows, cols = blocks.shape[:2]
    nat = np.zeros((rows * cols, 64), np.int64)
    nat[:, ZIGZAG] = blocks.reshape(-1, 64)
    px = idct_islow((nat * table[None, :]).reshape(-1, 8, 8))
    return px.reshape(rows, cols, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)


def upsample_h2v1(plane, dw):
    """jdsample.c h2v1_fancy_upsample over the first dw columns -> [rows, 2 dw]"""
    s = plane[:, :dw].astype(np.int64)
    if dw <= 2:
        return np.repeat(s, 2, 1)
    left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * dw), np.int64)
    out[:, 0::2] = (3 * s + left + 1) >> 2
    out[:, 1::2] = (3 * s + right + 2) >> 2
    out[:, 0], out[:, -1] = s[:, 0], s[:, -1]
    return out


def upsample_h2v2(plane, dh, dw):
    """jdsample.c h2v2_fancy_upsample over the first dh x dw samples -> [2 dh, 2 dw]"""
    s = plane[:dh, :dw].astype(np.int64)
    if dw <= 2:
        return np.repeat(np.repeat(s, 2, 0), 2, 1)
    above, below = np.concatenate([s[:1], s[:-1]]), np.concatenate([s[1:], s[-1:]])
    out = np.empty((2 * dh, 2 * dw), np.int64)
    for v, near in ((0, above), (1, below)):
        c = 3 * s + near
        left, right = np.concatenate([c[:, :1], c[:, :-1]], 1), np.concatenate([c[:, 1:], c[:, -1:]], 1)
        row = np.empty((dh, 2 * dw), np.int64)
        row[:, 0::2] = (3 * c + left + 8) >> 4
        row[:, 1::2] = (3 * c + right + 7) >> 4
        row[:, 0], row[:, -1] = (4 * c[:, 0] + 8) >> 4, (4 * c[:, -1] + 7) >> 4
        out[v::2] = row
    return out


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def pixels_of(blocks, hd, mode="RGB"):
    planes = [component_plane(b, hd.qt[c[2]]) for b, c in zip(blocks, hd.comps)]
    h, w = hd.h, hd.w
    if len(planes) == 1:
        grey = planes[0][:h, :w, None]
        return grey.copy() if mode == "unchanged" else np.repeat(grey, 3, 2)
    hs, vs = hd.comps[0][0], hd.comps[0][1]
    dh, dw = -(-h // vs), -(-w // hs)
    if (hs, vs) == (2, 2):
        cb, cr = (upsample_h2v2(p, dh, dw) for p in planes[1:])
    elif (hs, vs) == (2, 1):
        cb, cr = (upsample_h2v1(p[:h], dw) for p in planes[1:])
    else:
        cb, cr = planes[1], planes[2]
    return ycc_to_rgb(planes[0][:h, :w], cb[:h, :w], cr[:h, :w])


def decode(data, mode="RGB"):
    hd = parse(data)
    return pixels_of(decode_coefficients(data, hd), hd, mode)


# ------------------------------------------------------------------------------------------------
# the writer: a baseline file from given coefficients and tables
# ------------------------------------------------------------------------------------------------
def flat_tables():
    """Huffman tables that hold every symbol: DC sizes 0..11 as 4-bit codes, the 256 AC symbols as 8- and 9-bit codes."""
    dc = ([0, 0, 0, 12] + [0] * 12, list(range(12)))
    ac = ([0] * 7 + [128, 128] + [0] * 7, list(range(256)))
    return dc, ac


def write(blocks, h, w, sampling=(1, 1), qtables=None, dc_tables=None, ac_tables=None, ri=0, sof=0xC0, comment=b""):
    """blocks: per component int [block rows, block columns, 64] in zig-zag order, whole MCUs (1 or 3 components; the first
    has `sampling`, the others 1x1).  qtables: per component 64 steps in natural order (default 1).  dc_tables / ac_tables:
    (luma, chroma) as (bits, symbols) (default Annex K).  ri: MCUs per restart interval, 0 for none.  The file is assembled
    by tests/jpeg_ref.py's `write_file`, the writer of the encoder's reference: component k uses quantisation table k."""
    nc = len(blocks)
    data, _, _ = E.write_file(blocks, h, w, samp=[sampling] + [(1, 1)] * (nc - 1),
                              qtables=qtables if qtables is not None else [np.ones(64, np.int64)] * nc, tq=list(range(nc)),
                              tabs=[0] + [1] * (nc - 1), dc_tables=dc_tables or (E.DC_LUMA, E.DC_CHROMA),
                              ac_tables=ac_tables or (E.AC_LUMA, E.AC_CHROMA), ri=ri, sof=sof, comment=comment)
    return data
