"""TEST INFRASTRUCTURE - the checks of the device JPEG decoder (csrc/jpeg_decode.h) shared by the hipsim tests
(tests/test_sim_jpeg_decode.py) and the GPU tests (tests/test_gpu_jpeg_decode.py): every function takes the library, the
stream and the device to run on.

The oracle is tests/jpeg_decode_ref.py, a numpy restatement of libjpeg's decoder that tests/test_jpeg_decode_ref.py pins to
Pillow pixel for pixel.  Every device image must EQUAL the reference's.  Every decode here goes through `decode`, which
calls the C ABI on guarded buffers: the 0xA5 bytes behind the output and behind the workspace must be untouched, the scan
bytes and the tables unchanged, the status word zero."""
import functools
import io

import numpy as np
import torch

from hairfastgan_amd import _marshal as M
from hairfastgan_amd import image_utils as IU
from tests import jpeg_decode_ref as D
from tests import jpeg_ref as E
from tests.png_checks import smooth

GUARD = 37
SHAPES = [(1, 1), (8, 8), (7, 13), (16, 16), (17, 9), (9, 33), (24, 40), (37, 53)]
MODES = ["grey", 0, 1, 2]
QUALITIES = [10, 75, 95, 100]
SUB_BYTES = [4, 16, 0]  # 4: a subsequence is shorter than a symbol; 0: the default


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape).astype(np.uint8)


def picture(shape, mode, seed=5):
    return smooth(tuple(shape) + (1 if mode == "grey" else 3,), seed)


def pil_file(img, quality, mode, **kw):
    import PIL.Image

    img = np.asarray(img)
    buf = io.BytesIO()
    if quality is not None:
        kw["quality"] = quality
    if mode == "grey":
        PIL.Image.fromarray(img[:, :, 0] if img.ndim == 3 else img, "L").save(buf, format="JPEG", **kw)
    else:
        PIL.Image.fromarray(img, "RGB").save(buf, format="JPEG", subsampling=mode, **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def grid_files(shape, mode, quality):
    c = 1 if mode == "grey" else 3
    return [pil_file(picture(shape, mode, shape[1]), quality, mode), pil_file(noise(shape + (c,), shape[0] * 1000 + shape[1] + c), quality, mode)]


@functools.lru_cache(maxsize=None)
def reference(data, mode="RGB"):
    """the reference's pixels of a file, computed once and never written"""
    out = D.decode(data, mode)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------
# writer-built files
# ------------------------------------------------------------------------------------------------
def _grey_blocks(rows, cols):
    return np.zeros((rows, cols, 64), np.int64)


def extreme_dc():
    """DC +-1023 at a step of 8: the sample value +-1023 lies outside the signed 10-bit range in which libjpeg's range-limit
    table (index modulo 1024) and a saturation agree; Pillow's libjpeg-turbo saturates"""
    b = _grey_blocks(2, 2)
    b[:, :, 0] = [[1023, -1023], [500, -500]]
    b[0, 0, 1], b[1, 1, 8] = 40, -33
    return D.write([b], 16, 16, qtables=[np.full(64, 8)])


def extreme_ac():
    """AC coefficients of +-2047 (11 bits, which the Annex K tables cannot code) and +-1023 with tables that hold every symbol"""
    b = _grey_blocks(2, 3)
    b[0, 0, 1], b[0, 1, 2], b[0, 2, 5], b[1, 0, 63], b[1, 1, 1], b[1, 2, 3] = 2047, -2047, 1023, -1023, 2047, -2047
    b[1, 1, 0], b[1, 2, 0] = 2047, 100
    dc, ac = D.flat_tables()
    return D.write([b], 16, 24, dc_tables=(dc, dc), ac_tables=(ac, ac))


def extreme_colour():
    """4:2:0 with extreme luma and chroma coefficients, a step of 3"""
    rng = np.random.default_rng(11)
    y, cb, cr = _grey_blocks(4, 4), _grey_blocks(2, 2), _grey_blocks(2, 2)
    for blk in (y, cb, cr):
        blk[:, :, 0] = rng.integers(-340, 341, blk.shape[:2])
        blk[:, :, 1:4] = rng.choice([-1023, -300, 0, 0, 300, 1023], blk.shape[:2] + (3,))
    return D.write([y, cb, cr], 29, 27, sampling=(2, 2), qtables=[np.full(64, 3)] * 3)


EXTREME_FILES = {"dc1023_step8": extreme_dc, "ac2047_flat_tables": extreme_ac, "colour420_step3": extreme_colour}


def refused_files():
    """name -> (file, a word of the ValueError that refuses it)"""
    import PIL.Image

    img = picture((24, 40), 0)
    buf = io.BytesIO()
    PIL.Image.fromarray(img, "RGB").convert("CMYK").save(buf, format="JPEG")
    base = pil_file(img, 75, 0)
    at = base.index(b"\xFF\xDB") + 4
    wide = base[:at] + bytes([base[at] | 0x10]) + base[at + 1:]
    buf_png = io.BytesIO()
    PIL.Image.fromarray(img, "RGB").save(buf_png, format="PNG")
    return {"progressive": (pil_file(img, 75, 2, progressive=True), "progressive"),
            "4:1:1": (D.write([_grey_blocks(1, 4), _grey_blocks(1, 1), _grey_blocks(1, 1)], 8, 32, sampling=(4, 1)), "sampling factors"),  # Pillow's "4:1:1" writes 4:2:0
            "cmyk": (buf.getvalue(), "4 components"),
            "16-bit tables": (wide, "16-bit quantisation"),
            "not a jpeg": (buf_png.getvalue(), "not a JPEG")}


# ------------------------------------------------------------------------------------------------
# the decoder on guarded buffers
# ------------------------------------------------------------------------------------------------
def decode(L, st, device, files, sub_bytes=0, mode="RGB", f32=False, expect_status=None, scan_of=None):
    """files: file bytes of ONE geometry -> (uint8 [B,H,W,C] numpy, float32 [B,C,H,W] numpy or None, status [B,2]); every
    assertion that needs no reference.  expect_status: the scans are corrupt - the status words are returned, not asserted.
    scan_of: replaces the scan bytes of each file (malformed inputs)."""
    heads = [IU.parse_jpeg_header(d) for d in files]
    hd = heads[0]
    geom = (hd.height, hd.width, hd.components, hd.hs, hd.vs, hd.restart_interval)
    assert all((x.height, x.width, x.components, x.hs, x.vs, x.restart_interval) == geom for x in heads)
    h, w, nc, hs, vs, ri = geom
    b = len(files)
    oc = 1 if (nc == 1 and mode == "unchanged") else 3
    scans = [bytes(scan_of(d[x.scan_start:])) if scan_of else d[x.scan_start:] for d, x in zip(files, heads)]
    offs = np.cumsum([0] + [len(s) for s in scans]).astype(np.int64)
    longest = max(len(s) for s in scans)
    raw = np.frombuffer(b"".join(scans) + b"\xA5" * GUARD, np.uint8).copy()  # the bytes behind the scans are not FF, not 00
    scan_t = torch.from_numpy(raw).to(device)
    scan_before = scan_t.clone()
    off_t = torch.from_numpy(offs).to(device)
    tab_t = torch.from_numpy(np.stack([x.tables for x in heads])).to(device)
    tab_before = tab_t.clone()
    n_out = b * h * w * oc
    out = torch.full((n_out + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    outf = torch.full((n_out + GUARD,), -7.0, dtype=torch.float32, device=device) if f32 else None
    status = torch.full((2 * b + 2,), -1, dtype=torch.int32, device=device)
    ws_bytes = int(L.hf_jpeg_decode_workspace_bytes(b, h, w, nc, hs, vs, ri, longest))
    assert ws_bytes > 0
    ws = torch.full((ws_bytes // 8 + 2 + GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=device)
    M.check(L, L.hf_jpeg_decode_u8(out.data_ptr(), outf.data_ptr() if f32 else None, status.data_ptr(), scan_t.data_ptr(), len(raw) - GUARD,
                                   off_t.data_ptr(), longest, tab_t.data_ptr(), b, h, w, nc, hs, vs, ri, oc, sub_bytes, ws.data_ptr(),
                                   ws_bytes, st), "hf_jpeg_decode_u8")
    out, status, ws = out.cpu().numpy(), status.cpu().numpy(), ws.cpu().numpy()
    assert torch.equal(scan_t, scan_before) and torch.equal(tab_t, tab_before), "an input was written"
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
        assert (status[:, 1] >= 0).all() and (status[:, 1] <= 256).all(), status
    return out[:n_out].reshape(b, h, w, oc), outf, status


def where_differs(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} of {ref.size} bytes differ, first at (y, x, c) = {tuple(bad[0])}: {got[tuple(bad[0])]} for {ref[tuple(bad[0])]}"


def check_files(L, st, device, files, sub_bytes=0, mode="RGB"):
    """files of one geometry decode to the reference's pixels"""
    got, _, status = decode(L, st, device, files, sub_bytes, mode)
    for data, img in zip(files, got):
        ref = reference(data, mode)
        assert img.shape == ref.shape and np.array_equal(img, ref), (sub_bytes, where_differs(img, ref))
    return got, status


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
def check_grid(L, st, device, shape, mode):
    """the shape x mode x quality grid, every file at every subsequence length"""
    for q in QUALITIES:
        for sub in SUB_BYTES:
            check_files(L, st, device, grid_files(shape, mode, q), sub)


@functools.lru_cache(maxsize=None)
def windows_file(mode):
    return pil_file(noise((64, 96, 1 if mode == "grey" else 3), 3), 100, mode)


def check_windows(L, st, device):
    """64 x 96 noise at quality 100: at 4 bytes per lane the scan spans several windows of the workgroup (a window holds 256
    lanes), so the state, the partial symbol and the bytes carried from window to window are exercised, and a subsequence
    is shorter than a symbol; the number of passes is recorded and is more than one"""
    for mode in MODES:
        data = windows_file(mode)
        assert len(data) - IU.parse_jpeg_header(data).scan_start > 3 * 256 * 4
        for sub in SUB_BYTES:
            _, status = check_files(L, st, device, [data], sub)
            assert status[0, 1] >= 2, status


def check_flat(L, st, device):
    """a flat image: every block is a few bits, one subsequence holds many blocks (and most lanes' guesses are right)"""
    for mode in MODES:
        c = 1 if mode == "grey" else 3
        for sub in SUB_BYTES:
            check_files(L, st, device, [pil_file(np.full((40, 56, c), 97, np.uint8), 75, mode)], sub)
        y, x = np.mgrid[0:24, 0:40]
        check_files(L, st, device, [pil_file(np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], c, 2), 100, mode)])


def stuffed_at_boundaries(data, sub=4):
    """how many stuffed FF 00 pairs of the scan straddle a window boundary of the decoder at `sub` bytes per lane (the FF is
    the last raw byte of a window, the 00 the first of the next)"""
    scan = data[IU.parse_jpeg_header(data).scan_start:]
    step = 256 * sub - 16
    return sum(1 for k in range(step, len(scan), step) if scan[k - 1] == 0xFF and scan[k] == 0x00)


STUFFED_SEED = None


def find_stuffed_seed(limit=512):
    """the first seed whose 64 x 96 grey noise file at quality 100 has a stuffed FF 00 across a window boundary at 4 bytes per
    lane - searched with the header parser alone, once per session"""
    global STUFFED_SEED
    if STUFFED_SEED is None:
        STUFFED_SEED = next(s for s in range(limit) if stuffed_at_boundaries(pil_file(noise((64, 96, 1), s), 100, "grey")))
    return STUFFED_SEED


def check_stuffing(L, st, device):
    data = pil_file(noise((64, 96, 1), find_stuffed_seed()), 100, "grey")
    assert stuffed_at_boundaries(data) >= 1 and data.count(b"\xFF\x00") >= 20
    for sub in SUB_BYTES:
        check_files(L, st, device, [data], sub)


def check_custom_tables(L, st, device):
    for mode in MODES:
        check_files(L, st, device, [pil_file(picture((37, 53), mode), 75, mode, optimize=True)], 4)
        check_files(L, st, device, [pil_file(picture((37, 53), mode), 75, mode, optimize=True)])
        for step in (1, 255):
            check_files(L, st, device, [pil_file(picture((24, 40), mode), None, mode, qtables=[[step] * 64] * 2)])
    for name in sorted(EXTREME_FILES):
        for sub in SUB_BYTES:
            check_files(L, st, device, [EXTREME_FILES[name]()], sub)


def check_restart(L, st, device):
    """no DRI is every other check; here Ri = 1, Ri = 3, one interval per MCU row, and ten intervals (the RST index wraps)"""
    for mode in MODES:
        img = picture((37, 53), mode)
        for kw in ({"restart_marker_blocks": 1}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1}):
            data = pil_file(img, 90, mode, **kw)
            assert IU.parse_jpeg_header(data).restart_interval > 0
            for sub in (4, 0):
                check_files(L, st, device, [data], sub)
    data = pil_file(picture((80, 8), 0), 75, 0, restart_marker_rows=1)
    assert data.count(b"\xFF\xD0") == 2 and data.count(b"\xFF\xD7") == 1
    check_files(L, st, device, [data])
    data = pil_file(noise((150, 21, 3), 2), 100, 2, restart_marker_rows=1)  # ten intervals of noise
    check_files(L, st, device, [data], 4)


def check_batch(L, st, device):
    """a file decodes to the same bytes alone, with others of its geometry in any position, and twice"""
    files = [pil_file(picture((37, 53), 2, 20 + k), 75, 2) for k in range(3)] + [pil_file(noise((37, 53, 3), 1), 100, 2)]
    together, _, _ = decode(L, st, device, files)
    again, _, _ = decode(L, st, device, files)
    assert np.array_equal(together, again)
    flipped, _, _ = decode(L, st, device, files[::-1])
    assert np.array_equal(flipped[::-1], together)
    for k, data in enumerate(files):
        alone, _, _ = decode(L, st, device, [data])
        assert np.array_equal(alone[0], together[k]) and np.array_equal(alone[0], reference(data))


def check_float(L, st, device):
    """the float planes are byte / 255 in IEEE arithmetic: all 256 values, and the planes of a colour file"""
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    data = pil_file(ramp, None, "grey", qtables=[[1] * 64])
    u8, f, _ = decode(L, st, device, [data], f32=True)
    assert len(np.unique(u8)) >= 250  # a step of 1: nearly every value survives; the rest come from the colour file below
    assert f.dtype == np.float32 and np.array_equal(f[0].view(np.uint32), (u8[0].transpose(2, 0, 1).astype(np.float32) / np.float32(255)).view(np.uint32))
    data = pil_file(noise((37, 53, 3), 8), 95, 1)
    u8, f, _ = decode(L, st, device, [data], f32=True)
    assert np.array_equal(u8[0], reference(data)) and set(np.unique(u8)) == set(range(256))
    want = torch.from_numpy(u8[0].transpose(2, 0, 1).copy()).to(torch.float32).div(255).numpy()  # the CPU's division
    assert np.array_equal(f[0].view(np.uint32), want.view(np.uint32))
    lut = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.array_equal(f[0], lut[u8[0].transpose(2, 0, 1)])
    grey = pil_file(picture((17, 9), "grey"), 75, "grey")
    u1, f1, _ = decode(L, st, device, [grey], mode="unchanged", f32=True)
    assert u1.shape == (1, 17, 9, 1) and f1.shape == (1, 1, 17, 9) and np.array_equal(u1[0], reference(grey, "unchanged"))


def check_refusals():
    """header-level refusals need no kernel: each is a ValueError that names the cause"""
    for what, (data, word) in refused_files().items():
        try:
            IU.parse_jpeg_header(data)
        except ValueError as e:
            assert word in str(e), (what, e)
        else:
            raise AssertionError(f"{what}: must be refused")
    hd = IU.parse_jpeg_header(pil_file(picture((24, 40), 1), 75, 1, restart_marker_rows=1))
    assert (hd.height, hd.width, hd.components, hd.hs, hd.vs, hd.restart_interval) == (24, 40, 3, 2, 1, 3)
    assert hd.tables.shape == (M.JPEG_TABLE_BYTES,) and hd.tables.dtype == np.uint8


def check_invalid(L, st, device):
    data = pil_file(picture((24, 40), 2), 75, 2)
    hd = IU.parse_jpeg_header(data)
    scan = torch.from_numpy(np.frombuffer(data[hd.scan_start:], np.uint8).copy()).to(device)
    off = torch.tensor([0, scan.numel()], dtype=torch.int64, device=device)
    tab = torch.from_numpy(hd.tables[None].copy()).to(device)
    out = torch.zeros(24 * 40 * 3, dtype=torch.uint8, device=device)
    status = torch.full((2,), -1, dtype=torch.int32, device=device)
    n = scan.numel()
    ws_bytes = int(L.hf_jpeg_decode_workspace_bytes(1, 24, 40, 3, 2, 2, 0, n))
    ws = torch.zeros(ws_bytes // 8 + 4, dtype=torch.int64, device=device)
    f = L.hf_jpeg_decode_u8
    o, s, sc, of, tb, wp = out.data_ptr(), status.data_ptr(), scan.data_ptr(), off.data_ptr(), tab.data_ptr(), ws.data_ptr()
    invalid = {
        "no output": lambda: f(None, None, s, sc, n, of, n, tb, 1, 24, 40, 3, 2, 2, 0, 3, 0, wp, ws_bytes, st),
        "null status": lambda: f(o, None, None, sc, n, of, n, tb, 1, 24, 40, 3, 2, 2, 0, 3, 0, wp, ws_bytes, st),
        "null scans": lambda: f(o, None, s, None, n, of, n, tb, 1, 24, 40, 3, 2, 2, 0, 3, 0, wp, ws_bytes, st),
        "null offsets": lambda: f(o, None, s, sc, n, None, n, tb, 1, 24, 40, 3, 2, 2, 0, 3, 0, wp, ws_bytes, st),
        "null tables": lambda: f(o, None, s, sc, n, of, n, None, 1, 24, 40, 3, 2, 2, 0, 3, 0, wp, ws_bytes, st),
        "null workspace": lambda: f(o, None, s, sc, n, of, n, tb, 1, 24, 40, 3, 2, 2, 0, 3, 0, None, ws_bytes, st),
        "four components": lambda: f(o, None, s, sc, n, of, n, tb, 1, 24, 40, 4, 1, 1, 0, 3, 0, wp, ws_bytes, st),
        "4:1:1": lambda: f(o, None, s, sc, n, of, n, tb, 1, 24, 40, 3, 4, 1, 0, 3, 0, wp, ws_bytes, st),
        "4:4:0": lambda: f(o, None, s, sc, n, of, n, tb, 1, 24, 40, 3, 1, 2, 0, 3, 0, wp, ws_bytes, st),
        "grey 2x2": lambda: f(o, None, s, sc, n, of, n, tb, 1, 24, 40, 1, 2, 2, 0, 3, 0, wp, ws_bytes, st),
        "one channel of colour": lambda: f(o, None, s, sc, n, of, n, tb, 1, 24, 40, 3, 2, 2, 0, 1, 0, wp, ws_bytes, st),
        "no rows": lambda: f(o, None, s, sc, n, of, n, tb, 1, 0, 40, 3, 2, 2, 0, 3, 0, wp, ws_bytes, st),
        "width 65536": lambda: f(o, None, s, sc, n, of, n, tb, 1, 24, 65536, 3, 2, 2, 0, 3, 0, wp, ws_bytes, st),
        "no batch": lambda: f(o, None, s, sc, n, of, n, tb, 0, 24, 40, 3, 2, 2, 0, 3, 0, wp, ws_bytes, st),
        "sub_bytes 3": lambda: f(o, None, s, sc, n, of, n, tb, 1, 24, 40, 3, 2, 2, 0, 3, 3, wp, ws_bytes, st),
        "sub_bytes 65": lambda: f(o, None, s, sc, n, of, n, tb, 1, 24, 40, 3, 2, 2, 0, 3, 65, wp, ws_bytes, st),
        "restart interval -1": lambda: f(o, None, s, sc, n, of, n, tb, 1, 24, 40, 3, 2, 2, -1, 3, 0, wp, ws_bytes, st),
    }
    for what, call in invalid.items():
        try:
            M.check(L, call(), what)
        except RuntimeError as e:
            assert "invalid argument" in str(e), (what, e)
        else:
            raise AssertionError(f"{what}: must be refused")
    try:
        M.check(L, f(o, None, s, sc, n, of, n, tb, 1, 24, 40, 3, 2, 2, 0, 3, 0, wp, ws_bytes - 1, st), "short workspace")
    except RuntimeError as e:
        assert "code -3" in str(e), e
    else:
        raise AssertionError("short workspace: must be refused")
    assert not out.cpu().any() and (status.cpu() == -1).all()  # nothing was launched
    assert L.hf_jpeg_decode_workspace_bytes(1, 24, 40, 4, 1, 1, 0, n) == 0 and L.hf_jpeg_decode_workspace_bytes(0, 24, 40, 3, 2, 2, 0, n) == 0
    assert L.hf_jpeg_decode_workspace_bytes(1, 65535, 1, 1, 1, 1, 0, n) > 0 and L.hf_jpeg_decode_workspace_bytes(1, 24, 40, 3, 2, 2, 0, 1 << 31) == 0


def check_marshalled(L, st, device):
    """M.jpeg_decode: the same pixels as the guarded call"""
    files = [pil_file(picture((9, 21), 1, k), 92, 1) for k in range(2)]
    heads = [IU.parse_jpeg_header(d) for d in files]
    scans = [d[x.scan_start:] for d, x in zip(files, heads)]
    scan_t = torch.from_numpy(np.frombuffer(b"".join(scans), np.uint8).copy()).to(device)
    off_t = torch.tensor([0, len(scans[0]), len(scans[0]) + len(scans[1])], dtype=torch.int64, device=device)
    tab_t = torch.from_numpy(np.stack([x.tables for x in heads])).to(device)
    u8, f32, status = M.jpeg_decode(L, st, scan_t, off_t, max(map(len, scans)), tab_t, 9, 21, 3, 2, 1, 0, f32=True)
    assert not status[:, 0].cpu().any()
    assert np.array_equal(u8.cpu().numpy(), decode(L, st, device, files)[0])
    assert torch.equal(f32.cpu(), u8.cpu().permute(0, 3, 1, 2).to(torch.float32).div(255))


# ------------------------------------------------------------------------------------------------
# malformed scans: for the CPU interpreter only
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def malformed_cases():
    """name -> (file, replacement of its scan bytes)"""
    base = pil_file(noise((40, 56, 3), 4), 90, 2)
    rst = pil_file(noise((40, 56, 3), 4), 90, 2, restart_marker_rows=1)
    rng = np.random.default_rng(9)
    junk = bytes(rng.integers(0, 256, 40, dtype=np.uint8).tolist()).replace(b"\xFF", b"\xFE")
    dc, ac = D.flat_tables()
    short_ac = ([0, 2] + [0] * 14, [0x00, 0x01])  # the codes 00 and 01: 10 and 11 begin no code of the table
    absent = D.write([np.zeros((1, 1, 64), np.int64)], 8, 8, dc_tables=(dc, dc), ac_tables=(short_ac, short_ac))
    many = np.zeros((1, 1, 64), np.int64)
    many[0, 0, 1:61] = 1
    too_many = D.write([many], 8, 8, dc_tables=(dc, dc), ac_tables=(ac, ac))
    # coefficients 1..60, then in place of the EOB a symbol of run 5: its coefficient would be number 66
    hd = IU.parse_jpeg_header(too_many)
    length = E.huffman_codes(ac)[0x01][1]
    code, run_length = E.huffman_codes(ac)[0x51]
    bits = "".join(f"{x:08b}" for x in too_many[hd.scan_start:-2].replace(b"\xFF\x00", b"\xFF"))
    n_bits = 4 + 60 * (length + 1)
    bits = bits[:n_bits] + f"{code:0{run_length}b}" + "1"
    bits += "1" * (-len(bits) % 8)
    extra = bytes(int(bits[k:k + 8], 2) for k in range(0, len(bits), 8)).replace(b"\xFF", b"\xFF\x00") + b"\xFF\xD9"
    few = np.zeros((2, 2, 64), np.int64)
    too_few = D.write([few[:1]], 8, 16)  # the scan of an 8 x 16 image under the header of a 16 x 16 one
    few_head = D.write([few], 16, 16)
    hd_few, hd_head = IU.parse_jpeg_header(too_few), IU.parse_jpeg_header(few_head)
    return {
        "truncated at half": (base, lambda s: s[:len(s) // 2]),
        "truncated at the last byte": (base, lambda s: s[:-1]),
        "random bytes": (base, lambda s: junk + b"\xFF\xD9"),
        "random bytes with restart markers": (rst, lambda s: junk),
        "a code absent from the table": (absent, lambda s: bytes([0b00001100, 0x00]) + b"\xFF\xD9"),  # DC size 0, then 11...
        "more than 64 coefficients": (too_many, lambda s: extra),
        "a stray marker": (base, lambda s: s[:200].rstrip(b"\xFF") + b"\xFF\xC4" + s[200:]),
        "a wrong restart marker": (rst, lambda s: s.replace(b"\xFF\xD1", b"\xFF\xD5", 1)),
        "a missing restart marker": (rst, lambda s: s.replace(b"\xFF\xD1", b"\x12\x34", 1)),
        "too few MCUs": (few_head, lambda s: too_few[hd_few.scan_start:]),
        "an empty scan": (base, lambda s: b"\xFF\xD9"),
    }


def check_malformed(L, st, device, name):
    """an error status, never a write outside the buffers (`decode` checks the guards), at every subsequence length"""
    data, scan_of = malformed_cases()[name]
    try:
        D.decode(data if scan_of is None else data[:IU.parse_jpeg_header(data).scan_start] + bytes(scan_of(data[IU.parse_jpeg_header(data).scan_start:])))
    except ValueError:
        pass
    else:
        raise AssertionError(f"{name}: the reference decodes this file; it is not malformed")
    for sub in SUB_BYTES:
        _, _, status = decode(L, st, device, [data], sub, expect_status=True, scan_of=scan_of)
        assert 1 <= status[0, 0] <= 5, (name, sub, status)
