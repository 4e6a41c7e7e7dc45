"""TEST INFRASTRUCTURE - the checks of the device PNG decoder (csrc/png_decode.h) shared by the hipsim tests
(tests/test_sim_png_decode.py) and the GPU tests (tests/test_gpu_png_decode.py): every function takes the library, the
stream and the device to run on.

The reference is Pillow: `PIL.Image.open(io.BytesIO(f)).convert("RGB")`, and for "unchanged" the file's own mode (a palette
file expanded to RGB), byte for byte.  Files are made at test time: by PIL, by Python's zlib (`png_file` wraps any zlib
stream of hand-filtered rows into chunks), by the bit writer below (hand-assembled deflate blocks) and by this project's
encoder (tests/png_checks.encode).  Every decode goes through `decode`, which calls the C ABI on guarded buffers: the 0xA5
bytes behind the outputs and the 0x5A behind the workspace must be untouched, the streams unchanged.

`inflate_trace` is a small Python inflate that lists a stream's blocks and matches; the checks use it to assert that a file
holds what its case is about (a match of distance 32768 and length 258, a pattern inside Huffman data).  The malformed
streams are for the CPU interpreter only."""
import functools
import io
import struct
import zlib

import numpy as np
import torch

from hairfastgan_amd import _marshal as M
from hairfastgan_amd import image_utils as IU
from tests import png_checks as P

GUARD = 37
SHAPES = [(1, 1), (1, 2), (3, 5), (7, 13), (17, 9), (37, 53)]
COLOR_TYPES = [0, 2, 3, 4, 6]
PIL_MODES = {0: "L", 2: "RGB", 3: "P", 4: "LA", 6: "RGBA"}
TOKEN_CAPS = [2, 0]  # 2: the smallest token buffer, every match in a round of its own; 0: the default
BAND = 64            # rows of one band of the unfilter wavefront (kPdWave)
PATTERN = b"\x00\x00\xff\xff"


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------
def chunk(ctype, body):
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", zlib.crc32(ctype + body))


def png_file(h, w, color_type, stream, palette=None, splits=None, extra=()):
    """a PNG file around a zlib stream; splits: the lengths of the IDAT chunks before the last (0 allowed)"""
    out = P.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color_type, 0, 0, 0))
    if palette is not None:
        out += chunk(b"PLTE", bytes(np.asarray(palette, np.uint8).reshape(-1).tolist()))
    for ctype, body in extra:
        out += chunk(ctype, body)
    pos = 0
    for n in (splits or []):
        out += chunk(b"IDAT", stream[pos:pos + n])
        pos += n
    return out + chunk(b"IDAT", stream[pos:]) + chunk(b"IEND", b"")


def zlib_stream(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=(), flush_mode=zlib.Z_FULL_FLUSH):
    """raw bytes -> a zlib stream; flushes: positions of `raw` at which the compressor is flushed"""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    out, pos = b"", 0
    for at in flushes:
        out += co.compress(raw[pos:at]) + co.flush(flush_mode)
        pos = at
    return out + co.compress(raw[pos:]) + co.flush()


def adam7_file(img):
    """an interlaced (Adam7) RGB file of img, filter type None on every row of every pass: a file Pillow reads and the device
    decoder's header parser refuses"""
    h, w, _ = img.shape
    raw = bytearray()
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = img[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            for row in sub:
                raw += b"\x00" + row.tobytes()
    return P.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 1)) + chunk(b"IDAT", zlib.compress(bytes(raw), 1)) + chunk(b"IEND", b"")


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def filter_rows(pixels, types):
    """pixels uint8 [H,W,C], one filter type per row -> the filtered scanlines (the inflated bytes of the file)"""
    h, w, c = pixels.shape
    rows = pixels.reshape(h, w * c).astype(np.int64)
    out = bytearray()
    for y in range(h):
        cur, prev = rows[y], rows[y - 1] if y else np.zeros(w * c, np.int64)
        a = np.concatenate([np.zeros(c, np.int64), cur[:-c]]) if w * c > c else np.zeros(w * c, np.int64)
        cc = np.concatenate([np.zeros(c, np.int64), prev[:-c]]) if w * c > c else np.zeros(w * c, np.int64)
        t = types[y]
        if t == 0:
            pred = np.zeros(w * c, np.int64)
        elif t == 1:
            pred = a
        elif t == 2:
            pred = prev
        elif t == 3:
            pred = (a + prev) // 2
        else:
            pred = np.array([paeth(int(x), int(y_), int(z)) for x, y_, z in zip(a, prev, cc)], np.int64)
        out.append(t)
        out += bytes(((cur - pred) & 255).astype(np.uint8).tolist())
    return bytes(out)


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape).astype(np.uint8)


def picture(shape, c, seed=5):
    return P.smooth(tuple(shape) + (c,), seed)


@functools.lru_cache(maxsize=None)
def default_palette():
    return noise((256, 3), 77)


def pil_file(pixels, color_type, level=6, palette=None, **kw):
    """pixels uint8 [H,W,C of the colour type] written by PIL"""
    import PIL.Image

    pixels = np.asarray(pixels)
    mode = PIL_MODES[color_type]
    im = PIL.Image.fromarray(pixels[:, :, 0] if pixels.shape[2] == 1 else pixels, mode)
    if color_type == 3:
        im.putpalette(bytes(np.asarray(default_palette() if palette is None else palette).reshape(-1).tolist()))
    buf = io.BytesIO()
    im.save(buf, format="PNG", compress_level=level, **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def grid_files(shape, color_type):
    """PIL at levels 0, 1, 6, 9, and a Z_FIXED stream of the level-6 file's scanlines, for a smooth picture and for noise"""
    c = M.PNG_COLOR_CHANNELS[color_type]
    out = []
    for k, img in enumerate((picture(shape, c, shape[1] + color_type), noise(shape + (c,), shape[0] * 100 + shape[1] + color_type))):
        pal = default_palette() if color_type == 3 else None
        for level in (0, 1, 6, 9):
            out.append(pil_file(img, color_type, level))
        raw = filter_rows(img, [(y + k) % 5 for y in range(shape[0])])
        out.append(png_file(shape[0], shape[1], color_type, zlib_stream(raw, 6, zlib.Z_FIXED), pal))
    return out


@functools.lru_cache(maxsize=None)
def reference(data, mode="RGB"):
    """Pillow's pixels of a file, computed once and never written"""
    import PIL.Image

    with PIL.Image.open(io.BytesIO(data)) as im:
        im.load()
        if mode == "RGB" or im.mode == "P":
            out = np.asarray(im.convert("RGB"))
        else:
            out = np.asarray(im)
            out = out[:, :, None] if out.ndim == 2 else out
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------
# a bit writer and an inflate trace
# ------------------------------------------------------------------------------------------------
class BitWriter:
    """deflate's bit order: values LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits += [(value >> k) & 1 for k in range(n)]

    def code(self, value, n):
        self.bits += [(value >> (n - 1 - k)) & 1 for k in range(n)]

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def data(self):
        self.align()
        b = self.bits
        return bytes(sum(b[k + j] << j for j in range(8)) for k in range(0, len(b), 8))


def canonical(lengths):
    """code lengths -> {symbol: (code, length)}"""
    out, code = {}, 0
    for l in range(1, 16):
        for s, n in enumerate(lengths):
            if n == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def zlib_wrap(deflate, raw):
    return b"\x78\x01" + deflate + struct.pack(">I", zlib.adler32(raw))


class _Bits:
    def __init__(self, data):
        self.d, self.p = data, 0

    def take(self, n):
        v = 0
        for k in range(n):
            if self.p >> 3 >= len(self.d):
                raise ValueError("truncated")
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << k
            self.p += 1
        return v

    def sym(self, table):
        code, n = 0, 0
        while True:
            code, n = code << 1 | self.take(1), n + 1
            if (code, n) in table:
                return table[(code, n)]
            if n > 15:
                raise ValueError("no code")


def inflate_trace(stream):
    """a zlib stream -> (bytes, blocks): blocks is a list of (type, first bit, end bit, matches, bytes before the block) with matches (length, distance)"""
    br = _Bits(stream)
    br.p = 16
    out, blocks = bytearray(), []
    while True:
        at = br.p
        final, btype = br.take(1), br.take(2)
        matches, before = [], len(out)
        if btype == 0:
            br.p = (br.p + 7) // 8 * 8
            n, nn = br.take(16), br.take(16)
            assert n ^ nn == 0xFFFF
            out += stream[br.p // 8:br.p // 8 + n]
            br.p += 8 * n
        else:
            if btype == 1:
                ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dl = [5] * 32
            else:
                nl, nd, nc = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
                cl = [0] * 19
                for k in range(nc):
                    cl[CL_ORDER[k]] = br.take(3)
                ct = {v: s for s, v in canonical(cl).items()}
                lens = []
                while len(lens) < nl + nd:
                    s = br.sym(ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + br.take(2))
                    elif s == 17:
                        lens += [0] * (3 + br.take(3))
                    else:
                        lens += [0] * (11 + br.take(7))
                ll, dl = lens[:nl], lens[nl:]
            lt = {v: s for s, v in canonical(ll).items()}
            dt = {v: s for s, v in canonical(dl).items()}
            while True:
                s = br.sym(lt)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    n = LEN_BASE[s - 257] + br.take(LEN_EXTRA[s - 257])
                    d = br.sym(dt)
                    d = DIST_BASE[d] + br.take(DIST_EXTRA[d])
                    matches.append((n, d, len(out)))
                    for _ in range(n):
                        out.append(out[-d])
        blocks.append((btype, at, br.p, matches, before))
        if final:
            return bytes(out), blocks


def idat_stream(data):
    hd = IU.parse_png_header(data)
    return b"".join(data[at:at + n] for at, n in hd.idat)


# ------------------------------------------------------------------------------------------------
# the decoder on guarded buffers
# ------------------------------------------------------------------------------------------------
def decode(L, st, device, files, token_cap=0, mode="RGB", f32=False, expect_status=None, stream_of=None):
    """files: file bytes of ONE geometry -> (uint8 [B,H,W,C] numpy, float32 [B,C,H,W] numpy or None, status [B,2]); every
    assertion that needs no reference.  expect_status: the streams are corrupt - the status words are returned, not asserted.
    stream_of: replaces the zlib stream of each file (malformed inputs)."""
    heads = [IU.parse_png_header(d) for d in files]
    hd = heads[0]
    geom = (hd.height, hd.width, hd.color_type)
    assert all((x.height, x.width, x.color_type) == geom for x in heads)
    h, w, ct = geom
    b = len(files)
    oc = 3 if (mode == "RGB" or ct == 3) else hd.channels
    streams = [bytes(stream_of(idat_stream(d))) if stream_of else idat_stream(d) for d in files]
    offs = np.cumsum([0] + [len(s) for s in streams]).astype(np.int64)
    longest = max(len(s) for s in streams)
    raw = np.frombuffer(b"".join(streams) + b"\xA5" * GUARD, np.uint8).copy()
    stream_t = torch.from_numpy(raw).to(device)
    stream_before = stream_t.clone()
    off_t = torch.from_numpy(offs).to(device)
    pal_t = torch.from_numpy(np.stack([x.palette for x in heads])).to(device) if ct == 3 else None
    n_out = b * h * w * oc
    out = torch.full((n_out + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    outf = torch.full((n_out + GUARD,), -7.0, dtype=torch.float32, device=device) if f32 else None
    status = torch.full((2 * b + 2,), -1, dtype=torch.int32, device=device)
    ws_bytes = int(L.hf_png_decode_workspace_bytes(b, h, w, ct, longest))
    assert ws_bytes > 0
    ws = torch.full((ws_bytes // 8 + 2 + GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=device)
    M.check(L, L.hf_png_decode_u8(out.data_ptr(), outf.data_ptr() if f32 else None, status.data_ptr(), stream_t.data_ptr(), len(raw) - GUARD,
                                  off_t.data_ptr(), longest, pal_t.data_ptr() if ct == 3 else None, b, h, w, ct, oc, token_cap, ws.data_ptr(),
                                  ws_bytes, st), "hf_png_decode_u8")
    out, status, ws = out.cpu().numpy(), status.cpu().numpy(), ws.cpu().numpy()
    assert torch.equal(stream_t, stream_before), "an input was written"
    assert (ws.view(np.uint8)[(ws_bytes + 7) // 8 * 8:] == 0x5A).all(), "written past the workspace"
    assert (out[n_out:] == 0xA5).all(), "written past the images"
    assert (status[2 * b:] == -1).all(), "written past the status words"
    if f32:
        outf = outf.cpu().numpy()
        assert (outf[n_out:] == -7.0).all(), "written past the float images"
        outf = outf[:n_out].reshape(b, oc, h, w)
    status = status[:2 * b].reshape(b, 2)
    if expect_status is None:
        assert (status[:, 0] == 0).all(), status
        assert (status[:, 1] >= 1).all(), status
    return out[:n_out].reshape(b, h, w, oc), outf, status


def where_differs(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} of {ref.size} bytes differ, first at (y, x, c) = {tuple(bad[0])}: {got[tuple(bad[0])]} for {ref[tuple(bad[0])]}"


def check_files(L, st, device, files, token_cap=0, mode="RGB"):
    """files of one geometry decode to Pillow's pixels"""
    got, _, status = decode(L, st, device, files, token_cap, mode)
    for data, img in zip(files, got):
        ref = reference(data, mode)
        assert img.shape == ref.shape and np.array_equal(img, ref), (token_cap, mode, where_differs(img, ref))
    return got, status


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
def check_grid(L, st, device, shape, color_type):
    """the shape x colour type grid: every file at both token buffer sizes, in both modes"""
    files = grid_files(shape, color_type)
    for cap in TOKEN_CAPS:
        check_files(L, st, device, files, cap)
    check_files(L, st, device, files, 0, "unchanged")


def filter_pixels(h, w, c):
    """bytes that make Paeth's tie-breaks and Average's floor matter: 0, 255 and neighbours, in runs and alternations"""
    vals = np.array([0, 255, 1, 254, 0, 0, 255, 255, 128, 127, 2, 253], np.uint8)
    rng = np.random.default_rng(h * 7 + w)
    img = vals[rng.integers(0, len(vals), size=(h, w, c))]
    img[::3, ::2] = vals[(np.arange(h)[::3, None, None] + np.arange(c)) % len(vals)]
    return img


@functools.lru_cache(maxsize=None)
def filter_files(c):
    """one file per filter type on every row (the first row's Up / Average / Paeth see a row of zeros above) and one that
    cycles the types; BAND + 3 rows: more than one band of the wavefront, and a partial one"""
    ct = {1: 0, 2: 4, 3: 2, 4: 6}[c]
    h, w = BAND + 3, 11
    img = filter_pixels(h, w, c)
    files = [png_file(h, w, ct, zlib_stream(filter_rows(img, [t] * h))) for t in range(5)]
    files.append(png_file(h, w, ct, zlib_stream(filter_rows(img, [y % 5 for y in range(h)]))))
    files.append(png_file(h, w, ct, zlib_stream(filter_rows(img, [(4 - y) % 5 for y in range(h)]))))
    return files, img


def check_filters(L, st, device):
    for c in (1, 2, 3, 4):
        files, img = filter_files(c)
        got, _ = check_files(L, st, device, files, 0, "unchanged")
        for k in range(len(files)):
            assert np.array_equal(got[k], img), (c, k)  # and the pixels the rows were filtered from
    wide = filter_pixels(2, 2 * BAND + 5, 3)  # a row longer than the band is tall: the skew runs out inside the row
    check_files(L, st, device, [png_file(2, wide.shape[1], 2, zlib_stream(filter_rows(wide, [4, 3])))])


def check_palette(L, st, device):
    idx = noise((7, 13, 1), 3)
    check_files(L, st, device, [pil_file(idx, 3)])
    small = (noise((7, 13, 1), 4) & 7)
    pal4 = noise((4, 3), 5)
    raw = filter_rows(small, [0] * 7)
    short = png_file(7, 13, 3, zlib_stream(raw), pal4)
    assert (small > 3).any()
    got, _ = check_files(L, st, device, [short])
    assert (got[0][small[:, :, 0] > 3] == 0).all()  # an index beyond a short palette is black, as Pillow
    trns = png_file(7, 13, 3, zlib_stream(raw), np.concatenate([pal4, pal4]), extra=[(b"tRNS", bytes([0, 128, 255]))])
    check_files(L, st, device, [trns])
    check_files(L, st, device, [trns], mode="unchanged")
    grey_trns = png_file(3, 5, 0, zlib_stream(filter_rows(noise((3, 5, 1), 6), [1, 2, 4])), extra=[(b"tRNS", b"\x00\x07"), (b"gAMA", struct.pack(">I", 45455))])
    check_files(L, st, device, [grey_trns])


@functools.lru_cache(maxsize=None)
def split_case():
    img = picture((17, 9), 3, 2)
    raw = filter_rows(img, [y % 5 for y in range(17)])
    dyn = zlib_stream(raw, 9)
    stored = zlib_stream(raw, 0)
    _, blocks = inflate_trace(dyn)
    assert blocks[0][0] in (1, 2)
    mid = (blocks[0][1] + blocks[0][2]) // 16  # a byte in the middle of the Huffman data
    return img, dyn, stored, mid


def check_idat_structure(L, st, device):
    img, dyn, stored, mid = split_case()
    files = [png_file(17, 9, 2, dyn, splits=[1] * (len(dyn) - 1)),          # 1-byte IDATs
             png_file(17, 9, 2, dyn, splits=[mid, 0, 3]),                    # a zero-length IDAT; a split inside a code
             png_file(17, 9, 2, stored, splits=[2 + 3]),                     # between LEN and NLEN of the stored block
             png_file(17, 9, 2, dyn)]
    assert stored[2] == 1 and stored[3:5] == struct.pack("<H", len(stored) - 11)
    got, _ = check_files(L, st, device, files)
    assert all(np.array_equal(g, img) for g in got)


@functools.lru_cache(maxsize=None)
def long_run_file():
    """a run of one byte longer than 3 * 258: matches of distance 1 whose length exceeds the distance"""
    img = np.full((1, 1000, 1), 9, np.uint8)
    stream = zlib_stream(filter_rows(img, [0]), 9)
    _, blocks = inflate_trace(stream)
    assert sum(1 for b in blocks for n, d, _ in b[3] if d == 1 and n == 258) >= 3
    return png_file(1, 1000, 0, stream)


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def put_match(w, n, d, lc, dc):
    idx = 28 if n == 258 else max(k for k in range(28) if LEN_BASE[k] <= n)
    w.code(*lc[257 + idx])
    w.put(n - LEN_BASE[idx], LEN_EXTRA[idx])
    di = max(k for k in range(30) if DIST_BASE[k] <= d)
    w.code(*dc[di])
    w.put(d - DIST_BASE[di], DIST_EXTRA[di])


def put_tokens(w, tokens, ll, dl):
    """tokens: a byte (literal), (length, distance), or "E" (end of block), in the codes of the lengths ll / dl"""
    lc, dc = canonical(ll), canonical(dl)
    for t in tokens:
        if t == "E":
            w.code(*lc[256])
        elif isinstance(t, tuple):
            put_match(w, t[0], t[1], lc, dc)
        else:
            w.code(*lc[int(t)])


def fixed_block(tokens, final=1):
    w = BitWriter()
    w.put(final, 1), w.put(1, 2)
    put_tokens(w, tokens, FIXED_LL, FIXED_D)
    return w.data()


def limited_code(symbols, maxbits=7):
    """a complete code of at most maxbits for the symbols (the first get the shortest codes) -> lengths [19]"""
    lens = {s: maxbits for s in symbols}
    total = len(symbols)  # in units of 2^-maxbits
    for s in symbols:
        while lens[s] > 1 and total + (1 << (maxbits - lens[s])) <= (1 << maxbits):
            total += 1 << (maxbits - lens[s])
            lens[s] -= 1
    assert total == 1 << maxbits, (symbols, lens)
    return [lens.get(s, 0) for s in range(19)]


def run_length_code(lens):
    """code lengths -> [(code-length symbol, extra value, extra bits)] with the repeat codes 16, 17 and 18"""
    seq, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 11:
            n = min(run, 138)
            seq.append((18, n - 11, 7))
        elif v == 0 and run >= 3:
            n = min(run, 10)
            seq.append((17, n - 3, 3))
        elif v != 0 and run >= 4:
            seq.append((v, 0, 0))
            n = 1 + min(run - 1, 6)
            seq.append((16, n - 4, 2))
        else:
            n = 1
            seq.append((v, 0, 0))
        i += n
    return seq


def put_dynamic_header(w, final, ll, dl, seq=None, extra_hclen=0):
    """the header of a dynamic block; seq: the coded lengths (default: every length as itself, no repeat codes) -> the
    code-length code's lengths"""
    seq = [(v, 0, 0) for v in ll + dl] if seq is None else seq
    hist = {}
    for s, _, _ in seq:
        hist[s] = hist.get(s, 0) + 1
    cl = limited_code(sorted(hist, key=lambda s: (-hist[s], s)))
    cc = canonical(cl)
    w.put(final, 1), w.put(2, 2)
    w.put(len(ll) - 257, 5), w.put(len(dl) - 1, 5)
    ncl = max(4, max(k for k in range(19) if cl[CL_ORDER[k]]) + 1) + extra_hclen
    assert ncl <= 19
    w.put(ncl - 4, 4)
    for k in range(ncl):
        w.put(cl[CL_ORDER[k]], 3)
    for s, e, nb in seq:
        w.code(*cc[s])
        w.put(e, nb)
    return cl


def grey_row_file(raw, stream):
    """a one-row grey file whose inflated bytes are `raw` (the filter byte and the pixels)"""
    assert raw[0] <= 4 and zlib.decompress(stream) == bytes(raw)
    return png_file(1, len(raw) - 1, 0, stream)


@functools.lru_cache(maxsize=None)
def far_match_file():
    """grey 184 x 184: 184 * 185 = 34040 filtered bytes > 32768 + 258.  zlib itself never emits a distance above 32506
    (its window less MIN_LOOKAHEAD), so the stream is assembled: a stored block of the first 32769 bytes, then a fixed-Huffman
    block that begins with the match of length 258 at distance 32768 and ends with the rest as literals."""
    h = w = 184
    rng = np.random.default_rng(1)
    raw = (rng.integers(1, 128, h * (w + 1)) * 2).astype(np.uint8)
    head = (rng.integers(0, 128, 258) * 2 + 1).astype(np.uint8)
    for i in range(258):  # a filter byte of either place is a zero in both
        if (1 + i) % (w + 1) == 0 or (1 + 32768 + i) % (w + 1) == 0:
            head[i] = 0
    raw[1:259] = head
    raw[1 + 32768:259 + 32768] = head
    raw[::w + 1] = 0  # filter type None
    raw = bytes(raw.tolist())
    first = 1 + 32768
    deflate = b"\x00" + struct.pack("<HH", first, first ^ 0xFFFF) + raw[:first] + fixed_block([(258, 32768)] + list(raw[first + 258:]) + ["E"])
    stream = zlib_wrap(deflate, raw)
    assert zlib.decompress(stream) == raw
    return png_file(h, w, 0, stream), stream


def check_matches(L, st, device):
    for cap in TOKEN_CAPS:
        check_files(L, st, device, [long_run_file()], cap)
    data, stream = far_match_file()
    _, blocks = inflate_trace(stream)
    assert any(n == 258 and d == 32768 for b in blocks for n, d, _ in b[3]), "no match of distance 32768 and length 258"
    check_files(L, st, device, [data])


@functools.lru_cache(maxsize=None)
def hand_block_file():
    """A dynamic block assembled by hand: literal/length lengths 1..12, 14 and 15 (a plain Huffman tree of the weights
    2^(16 - length) is 15 deep), a code-length code with lengths up to 7, the repeat codes 16 (four 15s), 17 (three zeros)
    and 18, one run of eleven zeros that runs across the HLIT / HDIST boundary, and a distance code of a single symbol
    (symbol 6: distances 9..12, one bit)."""
    ll = [0] * 263
    ll[0:12] = range(1, 13)
    ll[12] = ll[16] = 14
    ll[254:258] = [15] * 4
    dl = [0] * 6 + [1]
    assert sum(2.0 ** -n for n in ll if n) == 1.0 and P.huffman_depth([2 ** (16 - n) for n in ll if n]) == 15
    seq = run_length_code(ll + dl)
    assert {16, 17, 18} <= {s for s, _, _ in seq}
    at, crossing = 0, False
    for s, e, _ in seq:
        n = 1 if s < 16 else (3 + e if s in (16, 17) else 11 + e)
        crossing |= at < len(ll) < at + n
        at += n
    assert crossing and at == len(ll) + len(dl)
    w = BitWriter()
    cl = put_dynamic_header(w, 1, ll, dl, seq)
    assert max(cl) == 7
    lits = [0] + list(range(1, 13)) + [16, 254, 255, 5, 5]
    put_tokens(w, lits + [(3, 10), 7, 3, "E"], ll, dl)
    raw = lits + lits[-10:-7] + [7, 3]
    return grey_row_file(raw, zlib_wrap(w.data(), bytes(raw)))


def check_hand_block(L, st, device):
    for cap in TOKEN_CAPS:
        check_files(L, st, device, [hand_block_file()], cap)


# ------------------------------------------------------------------------------------------------
# the segment route
# ------------------------------------------------------------------------------------------------
def check_encoder_files(L, st, device):
    """this project's own files: one segment per group of rows, each decoded by its own workgroup"""
    for c in (3, 1):
        r = P.segment_rows(L, 64, 37, c)
        imgs = np.stack([P.smooth((2 * r + 1, 37, c), 30 + k) for k in range(2)])
        files = P.encode(L, st, device, imgs)
        for cap in TOKEN_CAPS:
            got, status = check_files(L, st, device, files, cap, "unchanged")
            assert np.array_equal(got, imgs)
            assert (status[:, 1] == 3).all(), status


@functools.lru_cache(maxsize=None)
def flush_files():
    img = picture((17, 9), 3, 8)
    raw = filter_rows(img, [y % 5 for y in range(17)])
    row = 9 * 3 + 1
    full = zlib_stream(raw, 6, flushes=(3 * row, 8 * row, 8 * row + 5))
    rep = np.concatenate([noise((8, 20, 3), 9)] * 2)
    rraw = filter_rows(rep, [0] * 16)
    sync = zlib_stream(rraw, 9, flushes=(len(rraw) // 2,), flush_mode=zlib.Z_SYNC_FLUSH)
    assert full.count(PATTERN) == 3 and sync.count(PATTERN) == 1
    _, blocks = inflate_trace(sync)
    assert any(d > at - b[4] for b in blocks[1:] for n, d, at in b[3]), "no match reaches back across the flush"
    return png_file(17, 9, 2, full), png_file(16, 20, 2, sync)


def check_flushes(L, st, device):
    full, sync = flush_files()
    for cap in TOKEN_CAPS:
        _, status = check_files(L, st, device, [full], cap)
        assert status[0, 1] == 4, status  # three flushes: four segments
        _, status = check_files(L, st, device, [sync], cap)
        assert status[0, 1] == 1, status  # the serial route


@functools.lru_cache(maxsize=None)
def stored_pattern_file():
    """a level-0 file whose pixel bytes hold 00 00 FF FF - followed by 01 00 00 FF FF, a final empty stored block: the false
    candidate decodes without an error and must still be discarded"""
    img = noise((3, 12, 1), 12)
    img[1, 2:6, 0] = [0, 0, 255, 255]
    img[1, 6:11, 0] = [1, 0, 0, 255, 255]
    stream = zlib_stream(filter_rows(img, [0, 0, 0]), 0)
    assert stream.count(PATTERN) == 2 and stream[2] == 1  # one final stored block holds both
    return png_file(3, 12, 0, stream)


@functools.lru_cache(maxsize=None)
def huffman_pattern_file():
    """00 00 FF FF inside Huffman data.  Every literal 0..254 has its own value as its 8-bit code, 256 and 257 have 9 bits, the
    one distance code has one bit: the literals 80 00 7F and a match are the bits 1 0000000 00000000 0 1111111 111111111 0.
    The number of matches before them and of unused code-length-code entries is searched until the run is byte-aligned."""
    ll, dl = [8] * 255 + [0, 9, 9], [1]
    for extra in range(5):
        for m in range(8):
            w = BitWriter()
            put_dynamic_header(w, 1, ll, dl, extra_hclen=extra)
            tokens = [0] + [(3, 1)] * m + [17, 99, 0x80, 0x00, 0x7F, (3, 1), 5, 6, "E"]
            put_tokens(w, tokens, ll, dl)
            deflate = w.data()
            raw = [0] + [0] * (3 * m) + [17, 99, 0x80, 0x00, 0x7F] + [0x7F] * 3 + [5, 6]
            if PATTERN in deflate[:-1]:
                stream = zlib_wrap(deflate, bytes(raw))
                _, blocks = inflate_trace(stream)
                q = stream.index(PATTERN)
                assert blocks[0][0] == 2 and blocks[0][1] < 8 * q and 8 * (q + 4) < blocks[0][2]
                return grey_row_file(raw, stream)
    raise AssertionError("no aligned pattern found")


def check_false_candidates(L, st, device):
    for data in (stored_pattern_file(), huffman_pattern_file()):
        for cap in TOKEN_CAPS:
            _, status = check_files(L, st, device, [data], cap)
            assert status[0, 1] == 1, status


# ------------------------------------------------------------------------------------------------
# batch, float output, arguments
# ------------------------------------------------------------------------------------------------
def check_batch(L, st, device):
    """a file decodes to the same bytes alone, with others of its geometry in any position, and twice"""
    files = [pil_file(picture((37, 53), 3, 20 + k), 2, level) for k, level in enumerate((0, 1, 9))] + [pil_file(noise((37, 53, 3), 1), 2, 6)]
    files.append(png_file(37, 53, 2, zlib_stream(filter_rows(picture((37, 53), 3, 3), [4] * 37), 6, flushes=(800, 3000))))
    together, _, _ = decode(L, st, device, files)
    again, _, _ = decode(L, st, device, files)
    assert np.array_equal(together, again)
    flipped, _, _ = decode(L, st, device, files[::-1])
    assert np.array_equal(flipped[::-1], together)
    for k, data in enumerate(files):
        alone, _, _ = decode(L, st, device, [data])
        assert np.array_equal(alone[0], together[k]) and np.array_equal(alone[0], reference(data))


def check_float(L, st, device):
    """the float planes are byte / 255 in IEEE arithmetic: all 256 values, the planes of a colour file, a grey file as it is"""
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    u8, f, _ = decode(L, st, device, [pil_file(ramp, 0)], mode="unchanged", f32=True)
    assert np.array_equal(u8[0], ramp) and f.shape == (1, 1, 16, 16)
    assert np.array_equal(f[0].view(np.uint32), (ramp.transpose(2, 0, 1).astype(np.float32) / np.float32(255)).view(np.uint32))
    data = pil_file(noise((37, 53, 4), 8), 6)
    u8, f, _ = decode(L, st, device, [data], f32=True)
    assert np.array_equal(u8[0], reference(data)) and f.shape == (1, 3, 37, 53)
    want = torch.from_numpy(reference(data).copy()).permute(2, 0, 1) / 255  # the CPU's division
    assert np.array_equal(f[0].view(np.uint32), want.numpy().view(np.uint32))
    u4, f4, _ = decode(L, st, device, [data], mode="unchanged", f32=True)
    assert u4.shape == (1, 37, 53, 4) and f4.shape == (1, 4, 37, 53) and np.array_equal(u4[0], reference(data, "unchanged"))


def check_invalid(L, st, device):
    data = pil_file(picture((24, 40), 3), 2)
    s = idat_stream(data)
    stream_t = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).to(device)
    off = torch.tensor([0, len(s)], dtype=torch.int64, device=device)
    pal = torch.zeros((1, 256, 3), dtype=torch.uint8, device=device)
    out = torch.zeros(24 * 40 * 3, dtype=torch.uint8, device=device)
    status = torch.full((2,), -1, dtype=torch.int32, device=device)
    n = len(s)
    ws_bytes = int(L.hf_png_decode_workspace_bytes(1, 24, 40, 2, n))
    ws = torch.zeros(ws_bytes // 8 + 4, dtype=torch.int64, device=device)
    f = L.hf_png_decode_u8
    o, sp, sc, of, pp, wp = out.data_ptr(), status.data_ptr(), stream_t.data_ptr(), off.data_ptr(), pal.data_ptr(), ws.data_ptr()
    invalid = {
        "no output": lambda: f(None, None, sp, sc, n, of, n, None, 1, 24, 40, 2, 3, 0, wp, ws_bytes, st),
        "null status": lambda: f(o, None, None, sc, n, of, n, None, 1, 24, 40, 2, 3, 0, wp, ws_bytes, st),
        "null streams": lambda: f(o, None, sp, None, n, of, n, None, 1, 24, 40, 2, 3, 0, wp, ws_bytes, st),
        "null offsets": lambda: f(o, None, sp, sc, n, None, n, None, 1, 24, 40, 2, 3, 0, wp, ws_bytes, st),
        "null workspace": lambda: f(o, None, sp, sc, n, of, n, None, 1, 24, 40, 2, 3, 0, None, ws_bytes, st),
        "a palette file without palettes": lambda: f(o, None, sp, sc, n, of, n, None, 1, 24, 40, 3, 3, 0, wp, ws_bytes, st),
        "colour type 1": lambda: f(o, None, sp, sc, n, of, n, None, 1, 24, 40, 1, 3, 0, wp, ws_bytes, st),
        "colour type 5": lambda: f(o, None, sp, sc, n, of, n, pp, 1, 24, 40, 5, 3, 0, wp, ws_bytes, st),
        "one channel of colour": lambda: f(o, None, sp, sc, n, of, n, None, 1, 24, 40, 2, 1, 0, wp, ws_bytes, st),
        "four channels of RGB": lambda: f(o, None, sp, sc, n, of, n, None, 1, 24, 40, 2, 4, 0, wp, ws_bytes, st),
        "one channel of a palette": lambda: f(o, None, sp, sc, n, of, n, pp, 1, 24, 40, 3, 1, 0, wp, ws_bytes, st),
        "no rows": lambda: f(o, None, sp, sc, n, of, n, None, 1, 0, 40, 2, 3, 0, wp, ws_bytes, st),
        "no batch": lambda: f(o, None, sp, sc, n, of, n, None, 0, 24, 40, 2, 3, 0, wp, ws_bytes, st),
        "token_cap 1": lambda: f(o, None, sp, sc, n, of, n, None, 1, 24, 40, 2, 3, 1, wp, ws_bytes, st),
        "token_cap 2049": lambda: f(o, None, sp, sc, n, of, n, None, 1, 24, 40, 2, 3, 2049, wp, ws_bytes, st),
    }
    for what, call in invalid.items():
        try:
            M.check(L, call(), what)
        except RuntimeError as e:
            assert "invalid argument" in str(e), (what, e)
        else:
            raise AssertionError(f"{what}: must be refused")
    try:
        M.check(L, f(o, None, sp, sc, n, of, n, None, 1, 24, 40, 2, 3, 0, wp, ws_bytes - 1, st), "short workspace")
    except RuntimeError as e:
        assert "code -3" in str(e), e
    else:
        raise AssertionError("short workspace: must be refused")
    assert not out.cpu().any() and (status.cpu() == -1).all()  # nothing was launched
    assert L.hf_png_decode_workspace_bytes(1, 24, 40, 1, n) == 0 and L.hf_png_decode_workspace_bytes(0, 24, 40, 2, n) == 0
    assert L.hf_png_decode_workspace_bytes(1, 24, 40, 2, 1 << 31) == 0 and L.hf_png_decode_workspace_bytes(1, 1 << 16, 1 << 15, 0, n) == 0


def check_marshalled(L, st, device):
    """M.png_decode: the same pixels as the guarded call"""
    files = [pil_file(noise((9, 21, 1), k), 3) for k in range(2)]
    heads = [IU.parse_png_header(d) for d in files]
    streams = [idat_stream(d) for d in files]
    stream_t = torch.from_numpy(np.frombuffer(b"".join(streams), np.uint8).copy()).to(device)
    off_t = torch.tensor([0, len(streams[0]), len(streams[0]) + len(streams[1])], dtype=torch.int64, device=device)
    pal_t = torch.from_numpy(np.stack([x.palette for x in heads])).to(device)
    u8, f32, status = M.png_decode(L, st, stream_t, off_t, max(map(len, streams)), pal_t, 9, 21, 3, f32=True)
    assert not status[:, 0].cpu().any()
    assert np.array_equal(u8.cpu().numpy(), decode(L, st, device, files)[0])
    assert torch.equal(f32.cpu(), u8.cpu().permute(0, 3, 1, 2).to(torch.float32).div(255))


# ------------------------------------------------------------------------------------------------
# header refusals: no kernel
# ------------------------------------------------------------------------------------------------
def refused_files():
    """name -> (file, a word of the ValueError that refuses it)"""
    import PIL.Image

    img = picture((8, 12), 3)
    good = pil_file(img, 2)
    buf16, buf1, buf4, jpg = io.BytesIO(), io.BytesIO(), io.BytesIO(), io.BytesIO()
    PIL.Image.fromarray(img[:, :, 0].astype(np.uint16) << 8).save(buf16, format="PNG")
    PIL.Image.fromarray(img[:, :, 0] > 127).save(buf1, format="PNG")
    PIL.Image.fromarray(img[:, :, 0] & 15, "P").save(buf4, format="PNG", bits=4)
    PIL.Image.fromarray(img, "RGB").save(jpg, format="JPEG")
    laced = adam7_file(img)
    assert np.array_equal(reference(laced), img)
    bad_crc = good[:29] + bytes([good[29] ^ 1]) + good[30:]
    no_idat = P.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 12, 8, 8, 2, 0, 0, 0)) + chunk(b"IEND", b"")
    no_plte = png_file(2, 2, 3, zlib_stream(b"\x00\x00\x00" * 2))
    return {"16-bit": (buf16.getvalue(), "bit depth 16"), "1-bit": (buf1.getvalue(), "bit depth 1"), "4-bit": (buf4.getvalue(), "bit depth 4"),
            "interlaced": (laced, "interlace"), "a bad signature": (b"\x89PNX" + good[4:], "signature"), "a bad IHDR CRC": (bad_crc, "CRC of IHDR"),
            "no IDAT": (no_idat, "no IDAT"), "a JPEG file": (jpg.getvalue(), "signature"), "a palette file without PLTE": (no_plte, "PLTE"),
            "colour type 5": (P.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 12, 8, 8, 5, 0, 0, 0)) + good[33:], "colour type 5"),
            "a zero width": (P.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 0, 8, 8, 2, 0, 0, 0)) + good[33:], "zero dimension")}


def check_refusals():
    for what, (data, word) in refused_files().items():
        try:
            IU.parse_png_header(data)
        except ValueError as e:
            assert "unsupported PNG" in str(e) and word in str(e), (what, e)
        else:
            raise AssertionError(f"{what}: must be refused")


def check_header_fields():
    img = noise((7, 13, 1), 3)
    data = pil_file(img, 3)
    hd = IU.parse_png_header(data)
    assert (hd.height, hd.width, hd.color_type, hd.channels) == (7, 13, 3, 1)
    assert hd.palette.shape == (256, 3) and hd.palette.dtype == np.uint8 and np.array_equal(hd.palette, default_palette())
    assert hd.idat_bytes == sum(n for _, n in hd.idat) and all(data[at - 4:at] == b"IDAT" for at, _ in hd.idat)
    assert zlib.decompress(idat_stream(data)) == filter_rows(img, list(zlib.decompress(idat_stream(data))[::14]))
    split = png_file(7, 13, 0, zlib_stream(b"\x00" * 98), splits=[3, 0, 4])
    assert [n for _, n in IU.parse_png_header(split).idat][:3] == [3, 0, 4]
    for ct, c in M.PNG_COLOR_CHANNELS.items():
        assert IU.parse_png_header(pil_file(noise((2, 3, c), ct), ct)).channels == c


# ------------------------------------------------------------------------------------------------
# malformed streams: for the CPU interpreter only
# ------------------------------------------------------------------------------------------------
def _bits(*fields):
    """(value, bits): LSB first; (value, bits, "code"): a Huffman code, MSB first"""
    w = BitWriter()
    for v, n, *kind in fields:
        (w.code if kind else w.put)(v, n)
    return w.data()


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """name -> (file, replacement of its zlib stream, the error code)"""
    img = noise((5, 9, 1), 4)
    raw = filter_rows(img, [0, 1, 2, 3, 4])
    base = png_file(5, 9, 0, zlib_stream(raw, 6))
    stored = zlib_stream(raw, 0)
    pad = b"\x55" * 8  # bits behind the point of the error, so that it is not taken for the stream's end
    ll3, dl1 = [0] * 256 + [1, 1], [1]

    def dynamic(ll, dl, seq=None, tokens=(), nl=None, nd=None):
        w = BitWriter()
        if nl is None:
            put_dynamic_header(w, 1, ll, dl, seq)
            put_tokens(w, tokens, ll, dl)
        else:
            w.put(1, 1), w.put(2, 2), w.put(nl - 257, 5), w.put(nd - 1, 5), w.put(0, 4)
        return b"\x78\x01" + w.data() + pad

    first16 = [(16, 0, 2)] + [(1, 0, 0)] * 260  # "repeat the previous length" as the first symbol
    lit_bad = [8] * 255 + [0, 9, 9]
    return {
        "truncated at half": (base, lambda s: s[:len(s) // 2], 1),
        "no trailer": (base, lambda s: s[:-4], 1),
        "block type 3": (base, lambda s: b"\x78\x01" + _bits((1, 1), (3, 2)) + pad, 2),
        "stored LEN and NLEN": (base, lambda s: stored[:5] + bytes([stored[5] ^ 1]) + stored[6:], 3),
        "over-subscribed lengths": (base, lambda s: dynamic([0] * 255 + [1, 1, 1], dl1), 4),
        "incomplete lengths": (base, lambda s: dynamic([0] * 254 + [2, 2, 2], dl1), 4),
        "repeat without a previous length": (base, lambda s: dynamic(ll3 + [1, 1], dl1, first16), 5),
        "287 length codes": (base, lambda s: dynamic(None, None, nl=287, nd=1), 6),
        "a code not in the table": (base, lambda s: b"\x78\x01" + _dist_code_one(lit_bad) + pad, 7),
        "length symbol 286": (base, lambda s: b"\x78\x01" + _bits((1, 1), (1, 2), (0b11000110, 8, "code")) + pad, 8),
        "distance symbol 30": (base, lambda s: b"\x78\x01" + _bits((1, 1), (1, 2), (0b00110000, 8, "code"), (0b0000001, 7, "code"), (30, 5, "code")) + pad, 9),
        "a distance too far": (base, lambda s: b"\x78\x01" + fixed_block([7, (3, 5), "E"]) + pad, 10),
        "too many bytes": (base, lambda s: zlib_stream(raw + b"\x00" * 7, 6), 11),
        "too many bytes, stored": (base, lambda s: zlib_stream(raw + b"\x00" * 7, 0), 11),
        "too few bytes": (base, lambda s: zlib_stream(raw[:-5], 6), 12),
        "filter type 5": (base, lambda s: zlib_stream(raw[:10] + b"\x05" + raw[11:], 6), 13),
        "an Adler-32 that does not match": (base, lambda s: s[:-1] + bytes([s[-1] ^ 0x10]), 14),
        "compression method 9": (base, lambda s: b"\x79\x9c" + s[2:], 15),
        "a preset dictionary": (base, lambda s: b"\x78\x20" + s[2:], 15),
        "a wrong FCHECK": (base, lambda s: b"\x78\x02" + s[2:], 15),
    }


def _dist_code_one(ll):
    """literal 1, then a match whose distance code is the bit 1: the one distance code of the block is the bit 0"""
    w = BitWriter()
    put_dynamic_header(w, 1, ll, [1])
    lc = canonical(ll)
    w.code(*lc[1]), w.code(*lc[257]), w.put(1, 1)
    return w.data()


def check_malformed(L, st, device, name):
    """the case's error code, never a write outside the buffers (`decode` checks the guards), at both token buffer sizes"""
    data, stream_of, code = malformed_cases()[name]
    for cap in TOKEN_CAPS:
        _, _, status = decode(L, st, device, [data], cap, expect_status=True, stream_of=stream_of)
        assert status[0, 0] == code, (name, cap, status)
