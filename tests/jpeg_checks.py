"""TEST INFRASTRUCTURE - the checks of the device JPEG encoder (csrc/jpeg.h) shared by the hipsim tests
(tests/test_sim_jpeg.py) and the GPU tests (tests/test_gpu_jpeg.py): every function takes the library, the stream and the
device to run on.

The oracle is tests/jpeg_ref.py, a numpy restatement of libjpeg's pipeline that tests/test_jpeg_ref.py pins to Pillow byte
for byte.  Every device file must EQUAL the reference's bytes, open in PIL with `load()` in the right mode and size and
decode to the pixels the reference file decodes to; it is no longer than hf_jpeg_bound, and the 0xA5 bytes behind every slot,
behind the buffer and behind the workspace are untouched, the input unchanged.  Every encode here goes through `encode`, which
calls the C ABI on a guarded buffer whose slots start at odd addresses.  Where a case claims to reach a symbol or a code
path, that is asserted on the reference's histogram."""
import functools
import io

import numpy as np
import torch

from hairfastgan_amd import _marshal as M
from tests import jpeg_ref as R
from tests.png_checks import guarded_encode, smooth

SHAPES = [(1, 1), (8, 8), (7, 13), (16, 16), (17, 9), (9, 33), (24, 40), (37, 53)]  # 24x40: the padding-order case
MODES = ["grey", 0, 1, 2]
QUALITIES = [10, 75, 95, 100]
BLOCK_BITS = 11 + 11 + 63 * (16 + 10)  # the longest DC code and value, 63 times the longest AC code and value (Annex K tables)


def decode_pil(data):
    import PIL.Image

    with PIL.Image.open(io.BytesIO(data)) as im:
        im.load()
        return np.asarray(im), im.mode, im.size, im.format


def sub_of(mode):
    return 2 if mode == "grey" else mode


def scan_start(data):
    """Offset of the first entropy-coded byte: the marker segments walked from SOI to the end of SOS."""
    assert data[:2] == b"\xFF\xD8"
    pos = 2
    while True:
        assert data[pos] == 0xFF, (pos, data[pos])
        marker, pos = data[pos + 1], pos + 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
        if marker == 0xDA:
            return pos


@functools.lru_cache(maxsize=None)
def header_bytes(c):
    return scan_start(R.encode(np.zeros((1, 1, c), np.uint8), 75, 0).data)


def bound_from_tables(h, w, c, sub):
    """The largest file, derived as the header states it: every block at its longest code, every byte stuffed."""
    hs, vs = ((1, 1), (2, 1), (2, 2))[sub] if c == 3 else (1, 1)
    mcus, rows, nb = -(-w // (8 * hs)), -(-h // (8 * vs)), hs * vs + (2 if c == 3 else 0)
    return header_bytes(c) + rows * 2 * -(-mcus * nb * BLOCK_BITS // 8) + 2 * rows


# ------------------------------------------------------------------------------------------------
# the encoder on a guarded buffer
# ------------------------------------------------------------------------------------------------
def encode(L, st, device, images, quality=75, sub=2, base_offset=0):
    """images: numpy uint8 [B,H,W,C] -> list of file bytes; every structural assertion that needs no decoding."""
    images = np.ascontiguousarray(images)
    b, h, w, c = images.shape
    bound = int(L.hf_jpeg_bound(h, w, c, sub))
    assert 0 < bound <= bound_from_tables(h, w, c, sub), (bound, bound_from_tables(h, w, c, sub))  # no licence to waste
    ws_bytes = int(L.hf_jpeg_workspace_bytes(b, h, w, c, sub))
    return guarded_encode(L, device, images, "jpeg", bound, ws_bytes, lambda out, stride, sizes, src, ws: L.hf_jpeg_encode_u8(
        out, stride, sizes, src, b, h, w, c, quality, sub, ws, ws_bytes, st), base_offset)


def where_differs(got, ref):
    """A mismatch localised: the first differing byte and the restart interval (or header) it lies in."""
    at = next((k for k, (x, y) in enumerate(zip(got, ref.data)) if x != y), min(len(got), len(ref.data)))
    pos = scan_start(ref.data)
    if at < pos:
        return f"lengths {len(got)} / {len(ref.data)}, first difference at byte {at}, in the header"
    for k, iv in enumerate(ref.intervals):
        if at < pos + len(iv) + 2:
            return f"lengths {len(got)} / {len(ref.data)}, first difference at byte {at}: byte {at - pos} of interval {k} ({len(iv)} bytes)"
        pos += len(iv) + 2
    return f"lengths {len(got)} / {len(ref.data)}, first difference at byte {at}, behind the last interval"


def check_files(L, st, device, images, quality=75, sub=2, base_offset=0, refs=None):
    """The device files of the batch equal the reference's and decode like them; -> (files, references)."""
    images = np.ascontiguousarray(images)
    files = encode(L, st, device, images, quality, sub, base_offset)
    refs = refs if refs is not None else [R.encode(img, quality, sub) for img in images]
    for img, data, ref in zip(images, files, refs):
        assert data == ref.data, (img.shape, quality, sub, where_differs(data, ref))
        pixels, mode, size, fmt = decode_pil(data)
        assert fmt == "JPEG" and mode == ("RGB" if img.shape[2] == 3 else "L") and size == (img.shape[1], img.shape[0])
        assert np.array_equal(pixels, decode_pil(ref.data)[0])
    return files, refs


# ------------------------------------------------------------------------------------------------
# inputs and their references, made once
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiny_inputs(shape, c):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + c)
    return np.stack([smooth(shape + (c,), shape[1]), rng.integers(0, 256, size=shape + (c,)).astype(np.uint8)])


@functools.lru_cache(maxsize=None)
def tiny_refs(shape, c, quality, sub):
    return [R.encode(img, quality, sub) for img in tiny_inputs(shape, c)]


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape).astype(np.uint8)


def checkerboard():
    """8x8, one-pixel squares of 0 / 255: all the energy in the highest frequency."""
    y, x = np.mgrid[0:8, 0:8]
    return (((x + y) & 1) * 255).astype(np.uint8)[:, :, None]


def one_frequency(u, v, amplitude=100):
    """8x8 grey: 128 + amplitude * cos((2x+1) u pi / 16) * cos((2y+1) v pi / 16) - one AC coefficient."""
    y, x = np.mgrid[0:8, 0:8]
    img = 128 + amplitude * np.cos((2 * x + 1) * u * np.pi / 16) * np.cos((2 * y + 1) * v * np.pi / 16)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)[:, :, None]


def black_white_blocks(n=6):
    """8 x 8n grey: whole blocks of 0 and 255 in turn."""
    return np.repeat((np.arange(n) & 1) * 255, 8)[None, :].repeat(8, 0).astype(np.uint8)[:, :, None]


def blue_yellow_blocks(n=6):
    """8 x 8n RGB: whole blocks of (0, 0, 255) and (255, 255, 0) in turn - Cb swings between 255 and 0."""
    cols = np.repeat(np.arange(n) & 1, 8)
    return np.array([[0, 0, 255], [255, 255, 0]], np.uint8)[cols][None].repeat(8, 0)


def half_block():
    """8x8 grey, the left half black, the right half white."""
    img = np.zeros((8, 8, 1), np.uint8)
    img[:, 4:] = 255
    return img


PAD_FF_SEED = 14  # noise((8, 24, 1), seed) at quality 100: the padded last byte of the interval is FF (searched with jpeg_ref)


def find_pad_ff_seed(limit=4096):
    """How PAD_FF_SEED was found."""
    return next(s for s in range(limit) if R.encode(noise((8, 24, 1), s), 100, 0).hist["pad_ff"])


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
def check_tiny(L, st, device, shape, mode):
    c, sub = (1 if mode == "grey" else 3), sub_of(mode)
    for q in QUALITIES:
        check_files(L, st, device, tiny_inputs(shape, c), q, sub, refs=tiny_refs(shape, c, q, sub))


def restart_markers(data):
    """The RSTm indices of the scan, in file order (a stuffed FF 00 is no marker)."""
    scan = data[scan_start(data):-2]
    return [scan[k + 1] - 0xD0 for k in range(len(scan) - 1) if scan[k] == 0xFF and 0xD0 <= scan[k + 1] <= 0xD7]


def check_restart_wrap(L, st, device):
    for shape, sub in (((150, 21, 3), 2), ((80, 8, 3), 0)):
        img = smooth(shape, 7)[None]
        (data,), (ref,) = check_files(L, st, device, img, 75, sub)
        assert len(ref.intervals) == 10
        assert restart_markers(data) == [0, 1, 2, 3, 4, 5, 6, 7, 0], restart_markers(data)
        assert data[2 + 18 + 2 * 69 + 19 + 432:][:6] == b"\xFF\xDD\x00\x04" + (-(-shape[1] // (16 if sub else 8))).to_bytes(2, "big")


def chunk_mcus(L, c, sub):
    return int(L.hf_jpeg_chunk_mcus(c, sub))


def check_chunk_boundary(L, st, device):
    """An MCU row one MCU longer than the entropy kernel's chunk, and exact multiples of it: the bit offset and the partial
    byte carried from chunk to chunk (noise at quality 100: long codes, every carry length), ragged right and bottom edges."""
    assert [chunk_mcus(L, c, s) for c, s in ((1, 0), (3, 0), (3, 1), (3, 2))] == [256, 85, 64, 42]
    n = chunk_mcus(L, 3, 2)
    check_files(L, st, device, noise((1, 9, (n + 1) * 16 - 5, 3), 1), 100, 2)    # one MCU more; dummy blocks right and below
    check_files(L, st, device, smooth((16, n * 16, 3), 2)[None], 75, 2)          # exactly one chunk
    n = chunk_mcus(L, 3, 0)
    check_files(L, st, device, noise((1, 8, 2 * n * 8, 3), 3), 100, 0)           # exactly two chunks
    n = chunk_mcus(L, 1, 0)
    check_files(L, st, device, noise((1, 11, (n + 1) * 8 - 3, 1), 4), 95, 0)     # grey, one MCU more, two MCU rows
    n = chunk_mcus(L, 3, 1)
    check_files(L, st, device, noise((1, 8, (2 * n + 1) * 16, 3), 5), 100, 1)    # 4:2:2, two chunks and one MCU


def check_symbols(L, st, device):
    """Each input provably reaches its case: asserted on the reference's histogram, then the device file must equal it."""
    (_, ), (ref,) = check_files(L, st, device, checkerboard()[None], 100, 0)
    assert ref.hist["coef63"] >= 1 and ref.blocks[0][0, 0, 63] != 0          # no EOB: coefficient 63 is coded
    (_, ), (ref,) = check_files(L, st, device, one_frequency(7, 0)[None], 75, 0)
    assert ref.hist["zrl"] >= 1 and ref.hist["zrl_then_eob"] >= 1 and ref.blocks[0][0, 0, 63] == 0  # ZRL, a coefficient, EOB
    (_, ), (ref,) = check_files(L, st, device, one_frequency(7, 7)[None], 75, 0)
    assert ref.hist["zrl"] >= 3 and ref.hist["coef63"] >= 1                  # three ZRLs in front of coefficient 63
    (_, ), (ref,) = check_files(L, st, device, black_white_blocks()[None], 100, 0)
    assert ref.hist["dc11"] >= 4                                             # DC differences of 2040: size 11
    (_, ), (ref,) = check_files(L, st, device, blue_yellow_blocks()[None], 100, 0)
    assert np.abs(np.diff(ref.blocks[1][0, :, 0])).max() >= 1024             # size 11 with the chroma table: its 11-bit code
    for sub in (1, 2):
        check_files(L, st, device, blue_yellow_blocks()[None], 100, sub)
    (_, ), (ref,) = check_files(L, st, device, half_block()[None], 100, 0)
    assert ref.hist["ac10"] >= 1                                             # an AC coefficient of size 10
    img = noise((1, 40, 64, 3), 9)
    (data,), (ref,) = check_files(L, st, device, img, 100, 0)
    assert ref.hist["stuffed"] >= 50 and data.count(b"\xFF\x00") >= 50, ref.hist["stuffed"]
    (_, ), (ref,) = check_files(L, st, device, noise((1, 8, 24, 1), PAD_FF_SEED), 100, 0)
    assert ref.hist["pad_ff"] == 1 and ref.intervals[0].endswith(b"\xFF\x00")  # the padded last byte is FF, and stuffed


def check_bound(L, st, device):
    img = noise((1, 33, 97, 3), 3)
    (data,), _ = check_files(L, st, device, img, 100, 0)  # `encode` holds it to hf_jpeg_bound and checks the bytes behind it
    bound = int(L.hf_jpeg_bound(33, 97, 3, 0))
    assert img.size < len(data) <= bound, (len(data), bound)  # noise at quality 100 does not shrink
    assert L.hf_jpeg_bound(33, 97, 1, 0) == L.hf_jpeg_bound(33, 97, 1, 2) < L.hf_jpeg_bound(33, 97, 3, 2) < bound


def check_batch_invariance(L, st, device):
    imgs = np.stack([smooth((37, 53, 3), 20 + k) for k in range(3)])
    for q, sub in ((75, 2), (95, 0)):
        together = encode(L, st, device, imgs, q, sub)
        alone = [encode(L, st, device, imgs[k:k + 1], q, sub)[0] for k in range(3)]
        assert together == alone
        assert encode(L, st, device, imgs, q, sub) == together  # the same call twice
        assert encode(L, st, device, imgs, q, sub, base_offset=1) == together  # the bytes do not depend on where the input lies
    check_files(L, st, device, imgs, 75, 2)
    grey = imgs[:, :, :, :1]
    assert check_files(L, st, device, grey, 75, 0)[0] == encode(L, st, device, grey, 75, 2, base_offset=3)  # grey: one coding


def check_invalid(L, st, device):
    h, w, c = 5, 7, 3
    bound = int(L.hf_jpeg_bound(h, w, c, 2))
    ws_bytes = int(L.hf_jpeg_workspace_bytes(1, h, w, c, 2))
    img = torch.zeros(h * w * c, dtype=torch.uint8, device=device)
    out = torch.zeros(bound, dtype=torch.uint8, device=device)
    sizes = torch.zeros(1, dtype=torch.int64, device=device)
    ws = torch.zeros(ws_bytes // 8 + 4, dtype=torch.int64, device=device)
    o, s, i, wsp = out.data_ptr(), sizes.data_ptr(), img.data_ptr(), ws.data_ptr()
    assert wsp % 16 == 0
    f = L.hf_jpeg_encode_u8
    invalid = {
        "null out": lambda: f(None, bound, s, i, 1, h, w, c, 75, 2, wsp, ws_bytes, st),
        "null sizes": lambda: f(o, bound, None, i, 1, h, w, c, 75, 2, wsp, ws_bytes, st),
        "null in": lambda: f(o, bound, s, None, 1, h, w, c, 75, 2, wsp, ws_bytes, st),
        "null workspace": lambda: f(o, bound, s, i, 1, h, w, c, 75, 2, None, ws_bytes, st),
        "two channels": lambda: f(o, bound, s, i, 1, h, w, 2, 75, 2, wsp, ws_bytes, st),
        "four channels": lambda: f(o, bound, s, i, 1, h, w, 4, 75, 2, wsp, ws_bytes, st),
        "quality 0": lambda: f(o, bound, s, i, 1, h, w, c, 0, 2, wsp, ws_bytes, st),
        "quality 101": lambda: f(o, bound, s, i, 1, h, w, c, 101, 2, wsp, ws_bytes, st),
        "subsampling -1": lambda: f(o, bound, s, i, 1, h, w, c, 75, -1, wsp, ws_bytes, st),
        "subsampling 3": lambda: f(o, bound, s, i, 1, h, w, c, 75, 3, wsp, ws_bytes, st),
        "no batch": lambda: f(o, bound, s, i, 0, h, w, c, 75, 2, wsp, ws_bytes, st),
        "no rows": lambda: f(o, bound, s, i, 1, 0, w, c, 75, 2, wsp, ws_bytes, st),
        "width 65536": lambda: f(o, bound, s, i, 1, h, 65536, c, 75, 2, wsp, ws_bytes, st),
        "short stride": lambda: f(o, bound - 1, s, i, 1, h, w, c, 75, 2, wsp, ws_bytes, st),
    }
    for what, call in invalid.items():
        try:
            M.check(L, call(), what)
        except RuntimeError as e:
            assert "invalid argument" in str(e), (what, e)
        else:
            raise AssertionError(f"{what}: must be refused")
    try:
        M.check(L, f(o, bound, s, i, 1, h, w, c, 75, 2, wsp, ws_bytes - 1, st), "short workspace")
    except RuntimeError as e:
        assert "code -3" in str(e), e
    else:
        raise AssertionError("short workspace: must be refused")
    assert not out.cpu().any() and not sizes.cpu().any()  # nothing was launched
    assert L.hf_jpeg_bound(h, w, 2, 2) == 0 and L.hf_jpeg_bound(0, w, c, 2) == 0 and L.hf_jpeg_bound(h, 65536, c, 2) == 0
    assert L.hf_jpeg_bound(h, w, c, 3) == 0 and L.hf_jpeg_bound(65535, 65535, 3, 0) == 0  # a file of 2 GiB or more
    assert L.hf_jpeg_bound(65535, 1, 3, 2) > 0 and L.hf_jpeg_bound(1, 65535, 1, 0) > 0
    assert L.hf_jpeg_workspace_bytes(0, h, w, c, 2) == 0 and L.hf_jpeg_workspace_bytes(1, h, w, 4, 2) == 0
    assert L.hf_jpeg_chunk_mcus(2, 0) == 0 and L.hf_jpeg_chunk_mcus(3, 3) == 0
    for exc, call in [(TypeError, lambda: M.jpeg_encode(L, st, img.view(1, h, w, c).float())),
                      (ValueError, lambda: M.jpeg_encode(L, st, img.view(h, w, c))),
                      (ValueError, lambda: M.jpeg_encode(L, st, img[:h * w * 2].view(1, h, w, 2))),
                      (ValueError, lambda: M.jpeg_encode(L, st, img.view(1, h, w, c), 0)),
                      (ValueError, lambda: M.jpeg_encode(L, st, img.view(1, h, w, c), 75.0)),
                      (ValueError, lambda: M.jpeg_encode(L, st, img.view(1, h, w, c), 75, 3))]:
        try:
            call()
        except exc:
            pass
        else:
            raise AssertionError(f"expected {exc.__name__}")


def check_marshalled(L, st, device):
    """M.jpeg_encode: the same bytes as the guarded call."""
    imgs = np.stack([smooth((9, 21, 3), k) for k in range(2)])
    for q, sub in ((75, 2), (92, 1)):
        files, sizes = M.jpeg_encode(L, st, torch.from_numpy(imgs).to(device), q, sub)
        files, sizes = files.cpu().numpy(), sizes.cpu().numpy()
        assert [files[k, :sizes[k]].tobytes() for k in range(2)] == encode(L, st, device, imgs, q, sub)
