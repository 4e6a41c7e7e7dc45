"""TEST INFRASTRUCTURE - the checks of the device PNG encoder (csrc/png.h) shared by the hipsim tests (tests/test_sim_png.py)
and the GPU tests (tests/test_gpu_png.py): every function takes the library, the stream and the device to run on.

The oracle is two independent decoders:
1. `decode` below: the chunks split with `struct`, each CRC compared with `zlib.crc32(type + data)`, `zlib.decompress` of the
   IDAT (which verifies the Adler-32), the five PNG filters undone in numpy;
2. `PIL.Image.open(...).load()`.
Both must return exactly the input bytes, mode L / RGB and the input size; the file holds exactly IHDR, IDAT, IEND, is no
longer than hf_png_bound, and the 0xA5 bytes behind every slot and behind the buffer are untouched.  Every encode here goes
through `encode`, which calls the C ABI on a guarded buffer whose slots start at odd addresses."""
import functools
import heapq
import io
import struct
import zlib

import numpy as np
import torch

from hairfastgan_amd import _marshal as M

GUARD = 37          # bytes behind each slot (odd: the slots after the first start off every alignment)
SIGNATURE = b"\x89PNG\r\n\x1a\n"


# ------------------------------------------------------------------------------------------------
# decoders
# ------------------------------------------------------------------------------------------------
def chunks_of(data):
    assert data[:8] == SIGNATURE, data[:8]
    pos, out = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        ctype, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(ctype + body), (ctype, hex(crc), hex(zlib.crc32(ctype + body)))
        out.append((ctype, body))
        pos += 12 + n
    assert pos == len(data)
    return out


def _paeth(a, b, c):
    p = a.astype(np.int32) + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def decode(data):
    """-> (pixels uint8 [H,W,C], filter byte of every row)."""
    chunks = chunks_of(data)
    assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"], [c[0] for c in chunks]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (0, 2) and chunks[2][1] == b""
    assert chunks[1][1][:2] == b"\x78\x01"
    c = 3 if ctype == 2 else 1
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8)
    assert raw.size == h * (w * c + 1), (raw.size, h, w, c)
    rows = raw.reshape(h, w * c + 1)
    out = np.zeros((h, w * c), np.int32)
    prev = np.zeros(w * c, np.int32)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        assert ft <= 4, ft
        if ft in (0, 2):
            cur = (line + (prev if ft == 2 else 0)) & 255
        else:
            cur = np.zeros(w * c, np.int32)
            for i in range(w):  # pixel by pixel: the left neighbour is a decoded value
                sl = slice(i * c, i * c + c)
                a = cur[(i - 1) * c:i * c] if i else np.zeros(c, np.int32)
                b = prev[sl]
                cc = prev[(i - 1) * c:i * c] if i else np.zeros(c, np.int32)
                pred = a if ft == 1 else (a + b) // 2 if ft == 3 else _paeth(a, b, cc)
                cur[sl] = (line[sl] + pred) & 255
        out[y] = prev = cur
    return out.astype(np.uint8).reshape(h, w, c), rows[:, 0].copy()


def decode_pil(data):
    import PIL.Image

    with PIL.Image.open(io.BytesIO(data)) as im:
        im.load()
        return np.asarray(im), im.mode, im.size


# ------------------------------------------------------------------------------------------------
# the encoder on a guarded buffer
# ------------------------------------------------------------------------------------------------
def segment_rows(L, h, w, c):
    return int(L.hf_png_segment_rows(h, w, c))


def guarded_encode(L, device, images, codec, bound, ws_bytes, call, base_offset=0):
    """The guarded-buffer protocol of the codecs' `encode`: images (numpy uint8 [B,H,W,C], contiguous) at `base_offset` inside
    16 bytes, 0xA5 behind every slot of `bound` bytes and behind the buffer, 0x5A behind the workspace of `ws_bytes`;
    call(files, stride, sizes, source, workspace) -> the status of hf_<codec>_encode_u8.  The input is unchanged, the sizes
    lie within the bound, nothing is written past a file's own length; -> list of file bytes."""
    b = images.shape[0]
    stride = bound + GUARD
    src = torch.zeros(images.size + base_offset, dtype=torch.uint8, device=device)
    src[base_offset:] = torch.from_numpy(images.reshape(-1)).to(device)
    view = src[base_offset:]
    assert view.data_ptr() % 16 == base_offset % 16
    before = view.clone()
    files = torch.full((b * stride + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    sizes = torch.full((b,), -1, dtype=torch.int64, device=device)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes // 8 + 2 + GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=device)
    M.check(L, call(files.data_ptr(), stride, sizes.data_ptr(), view.data_ptr(), ws.data_ptr()), f"hf_{codec}_encode_u8")
    files, sizes, ws = files.cpu().numpy(), sizes.cpu().numpy(), ws.cpu().numpy()
    assert torch.equal(view, before), "the input was written"
    assert (ws.view(np.uint8)[(ws_bytes + 7) // 8 * 8:] == 0x5A).all(), "written past the workspace"
    assert (files[b * stride:] == 0xA5).all(), "written past the buffer"
    out = []
    for i in range(b):
        assert 0 < sizes[i] <= bound, (i, sizes[i], bound)
        slot = files[i * stride:(i + 1) * stride]
        assert (slot[bound:] == 0xA5).all(), f"image {i}: written past hf_{codec}_bound"
        assert (slot[sizes[i]:bound] == 0xA5).all(), f"image {i}: written past its own length"
        out.append(slot[:sizes[i]].tobytes())
    return out


def encode(L, st, device, images, filter_mode=3, base_offset=0):
    """images: numpy uint8 [B,H,W,C] -> list of file bytes; every structural assertion that needs no decoding."""
    images = np.ascontiguousarray(images)
    b, h, w, c = images.shape
    bound = int(L.hf_png_bound(h, w, c))
    r = segment_rows(L, h, w, c)
    n = h * (w * c + 1)
    assert 0 < bound <= n + 5 * -(-n // 65535) + 5 * -(-h // r) + 128, (bound, n, r)  # the bound is no licence to waste
    ws_bytes = int(L.hf_png_workspace_bytes(b, h, w, c))
    return guarded_encode(L, device, images, "png", bound, ws_bytes, lambda out, stride, sizes, src, ws: L.hf_png_encode_u8(
        out, stride, sizes, src, b, h, w, c, filter_mode, ws, ws_bytes, st), base_offset)


def check_roundtrip(L, st, device, images, filter_mode=3, base_offset=0):
    """Both decoders return the input; -> (files, filter bytes of each image)."""
    images = np.ascontiguousarray(images)
    files = encode(L, st, device, images, filter_mode, base_offset)
    rows = []
    for img, data in zip(images, files):
        got, ft = decode(data)
        assert got.shape == img.shape and np.array_equal(got, img), (img.shape, filter_mode, int((got != img).sum()))
        pil, mode, size = decode_pil(data)
        assert mode == ("RGB" if img.shape[2] == 3 else "L") and size == (img.shape[1], img.shape[0])
        assert np.array_equal(pil.reshape(img.shape), img)
        if filter_mode < 3:
            assert (ft == filter_mode).all(), (filter_mode, ft)
        rows.append(ft)
    return files, rows


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def smooth(shape, seed):
    """Random smooth data: a random walk along each row plus a slow drift down the rows, a little noise."""
    h, w, c = shape
    rng = np.random.default_rng(seed)
    walk = np.cumsum(rng.integers(-3, 4, size=(h, w, c)), axis=1) + np.cumsum(rng.integers(-2, 3, size=(h, 1, c)), axis=0)
    return ((walk + 128 + rng.integers(0, 2, size=(h, w, c))) & 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def photo(n):
    """The size probe's photograph: 128 + 90 sin(x/97 + y/53) + 20 sin(x/7.3) cos(y/5.1), the two sibling channels with the
    phases moved by 1 and 2, plus N(0, 3) noise, seed 0."""
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    rng = np.random.default_rng(0)
    ch = [128 + 90 * np.sin(x / 97 + y / 53 + k) + 20 * np.sin(x / 7.3 + k) * np.cos(y / 5.1) for k in range(3)]
    img = np.stack(ch, -1) + rng.normal(0, 3, size=(n, n, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def label_image(n):
    """The size probe's label map: (x // 37 + y // 91) % 19 through a random palette, seed 0."""
    y, x = np.mgrid[0:n, 0:n]
    palette = np.random.default_rng(0).integers(0, 256, size=(19, 3)).astype(np.uint8)
    return palette[(x // 37 + y // 91) % 19]


def pil_png_size(img, level):
    import PIL.Image

    buf = io.BytesIO()
    PIL.Image.fromarray(img if img.shape[2] == 3 else img[:, :, 0]).save(buf, format="PNG", compress_level=level)
    return buf.tell()


def huffman_depth(counts):
    """Depth of a plain (unlimited) Huffman tree of the counts."""
    heap = [(c, 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        (c1, d1), (c2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (c1 + c2, max(d1, d2) + 1))
    return heap[0][1]


def deep_code_row():
    """One grey row whose byte histogram is 2, 3, then f(i) = f(i-1) + f(i-2) + 1 (17 values, 15106 bytes), no byte equal to
    its predecessor: with the filter byte (0, once) and the end-of-block symbol (once) a tie-free histogram whose plain
    Huffman tree is 18 deep.  The encoder keeps a row of 15107 filtered bytes in ONE block (hf_png_segment_rows = 1 and the
    row fits a segment), so one construction covers the row."""
    counts = [2, 3]
    while len(counts) < 17:
        counts.append(counts[-1] + counts[-2] + 1)
    assert counts[-1] == 5777 and sum(counts) == 15106
    order = sorted(range(17), key=lambda k: -counts[k])  # the classic rearrangement: even places first, then odd ones
    flat = np.concatenate([np.full(counts[k], k + 1, np.uint8) for k in order])
    row = np.zeros(15106, np.uint8)
    half = (row.size + 1) // 2
    row[0::2], row[1::2] = flat[:half], flat[half:]
    assert (row[1:] != row[:-1]).all() and row[0] != 0
    assert np.array_equal(np.bincount(row, minlength=18)[1:], counts)
    return row.reshape(1, 15106, 1), [1, 1] + counts


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
TINY = [(1, 1, 1), (1, 1, 3), (1, 2, 3), (3, 5, 1), (7, 13, 3)]


def check_tiny(L, st, device, shape):
    rng = np.random.default_rng(sum(shape))
    check_roundtrip(L, st, device, rng.integers(0, 256, size=(1,) + shape).astype(np.uint8))
    check_roundtrip(L, st, device, smooth(shape, 1)[None])


def check_heights(L, st, device):
    r = segment_rows(L, 64, 13, 3)
    assert r >= 2 and all(segment_rows(L, h, 13, 3) == min(r, h) for h in (r - 1, r, r + 1, 2 * r + 1))
    for h in (r - 1, r, r + 1, 2 * r + 1):
        check_roundtrip(L, st, device, smooth((h, 13, 3), h)[None])


def check_offset_base(L, st, device):
    r = segment_rows(L, 64, 37, 3)
    img = smooth((2 * r + 1, 37, 3), 5)[None]
    aligned = check_roundtrip(L, st, device, img)[0]
    assert check_roundtrip(L, st, device, img, base_offset=1)[0] == aligned  # the bytes do not depend on where the input lies


def filter_case(L):
    r = segment_rows(L, 64, 37, 3)
    return smooth((2 * r + 1, 37, 3), 11)[None]


def check_filter(L, st, device, mode):
    _, rows = check_roundtrip(L, st, device, filter_case(L), mode)
    if mode == 3:
        assert len(set(rows[0].tolist())) > 1, rows  # smooth data: not one type on every row


def check_runs(L, st, device):
    for c in (3, 1):
        for value in (0, 0x7F):
            img = np.full((1, 40, 600, c), value, np.uint8)
            (data,), _ = check_roundtrip(L, st, device, img, 0)
            assert len(data) < img.size // 50, (c, value, len(data))  # runs are coded as runs
    widths = [1, 2, 3, 4, 259]
    cols = np.concatenate([np.full(wd, k & 1, np.uint8) for k, wd in enumerate(widths * 3)])
    colours = np.array([[10, 200, 30], [250, 0, 99]], np.uint8)
    stripes = np.broadcast_to(colours[cols][None], (9, cols.size, 3))
    for mode in (0, 1, 3):
        check_roundtrip(L, st, device, stripes[None], mode)
    check_roundtrip(L, st, device, np.broadcast_to((cols * 255)[None, :, None], (9, cols.size, 1))[None], 0)


def check_incompressible(L, st, device):
    img = np.random.default_rng(3).integers(0, 256, size=(1, 33, 97, 3)).astype(np.uint8)
    for mode in (0, 3):
        (data,), _ = check_roundtrip(L, st, device, img, mode)  # `encode` holds it to hf_png_bound
        assert len(data) >= img.size  # nothing to gain: the stored blocks


def check_deep_code(L, st, device):
    img, hist = deep_code_row()
    assert huffman_depth(hist) >= 16, huffman_depth(hist)
    assert segment_rows(L, 1, 15106, 1) == 1
    (data,), _ = check_roundtrip(L, st, device, img[None], 0)
    assert len(data) < img.size // 2  # a dynamic block, not the stored fallback (the entropy is 2.6 bits a byte)


def check_batch_invariance(L, st, device):
    r = segment_rows(L, 64, 37, 3)
    imgs = np.stack([smooth((2 * r + 1, 37, 3), 20 + k) for k in range(3)])
    for mode in (1, 3):
        together = encode(L, st, device, imgs, mode)
        alone = [encode(L, st, device, imgs[k:k + 1], mode)[0] for k in range(3)]
        assert together == alone
        assert encode(L, st, device, imgs, mode) == together  # the same call twice
    check_roundtrip(L, st, device, imgs)


def check_sizes(L, st, device):
    """256^2, adaptive filter: the photograph no larger than PIL compress_level=1, the label map at most 2 % of its bytes."""
    ph, lab = photo(256), label_image(256)
    (fp,), _ = check_roundtrip(L, st, device, ph[None])
    (fl,), _ = check_roundtrip(L, st, device, lab[None])
    p1, p6 = pil_png_size(ph, 1), pil_png_size(ph, 6)
    print(f"photo 256^2: device {len(fp)} B, PIL level 1 {p1} B (ratio {len(fp) / p1:.3f}), level 6 {p6} B")
    print(f"labels 256^2: device {len(fl)} B = {100 * len(fl) / lab.size:.2f} % of {lab.size} B; "
          f"PIL level 1 {pil_png_size(lab, 1)} B, level 6 {pil_png_size(lab, 6)} B")
    assert len(fp) <= p1, (len(fp), p1)
    assert len(fl) <= 0.02 * lab.size, (len(fl), lab.size)


def check_invalid(L, st, device):
    h, w, c = 5, 7, 3
    bound = int(L.hf_png_bound(h, w, c))
    ws_bytes = int(L.hf_png_workspace_bytes(1, h, w, c))
    img = torch.zeros(h * w * c, dtype=torch.uint8, device=device)
    out = torch.zeros(bound, dtype=torch.uint8, device=device)
    sizes = torch.zeros(1, dtype=torch.int64, device=device)
    ws = torch.zeros(ws_bytes // 8 + 4, dtype=torch.int64, device=device)
    o, s, i, wsp = out.data_ptr(), sizes.data_ptr(), img.data_ptr(), ws.data_ptr()
    assert wsp % 16 == 0
    invalid = {
        "null out": lambda: L.hf_png_encode_u8(None, bound, s, i, 1, h, w, c, 3, wsp, ws_bytes, st),
        "null sizes": lambda: L.hf_png_encode_u8(o, bound, None, i, 1, h, w, c, 3, wsp, ws_bytes, st),
        "null in": lambda: L.hf_png_encode_u8(o, bound, s, None, 1, h, w, c, 3, wsp, ws_bytes, st),
        "null workspace": lambda: L.hf_png_encode_u8(o, bound, s, i, 1, h, w, c, 3, None, ws_bytes, st),
        "two channels": lambda: L.hf_png_encode_u8(o, bound, s, i, 1, h, w, 2, 3, wsp, ws_bytes, st),
        "four channels": lambda: L.hf_png_encode_u8(o, bound, s, i, 1, h, w, 4, 3, wsp, ws_bytes, st),
        "filter 4": lambda: L.hf_png_encode_u8(o, bound, s, i, 1, h, w, c, 4, wsp, ws_bytes, st),
        "filter -1": lambda: L.hf_png_encode_u8(o, bound, s, i, 1, h, w, c, -1, wsp, ws_bytes, st),
        "no batch": lambda: L.hf_png_encode_u8(o, bound, s, i, 0, h, w, c, 3, wsp, ws_bytes, st),
        "no rows": lambda: L.hf_png_encode_u8(o, bound, s, i, 1, 0, w, c, 3, wsp, ws_bytes, st),
        "negative width": lambda: L.hf_png_encode_u8(o, bound, s, i, 1, h, -1, c, 3, wsp, ws_bytes, st),
        "short stride": lambda: L.hf_png_encode_u8(o, bound - 1, s, i, 1, h, w, c, 3, wsp, ws_bytes, st),
    }
    for what, call in invalid.items():
        try:
            M.check(L, call(), what)
        except RuntimeError as e:
            assert "invalid argument" in str(e), (what, e)
        else:
            raise AssertionError(f"{what}: must be refused")
    try:
        M.check(L, L.hf_png_encode_u8(o, bound, s, i, 1, h, w, c, 3, wsp, ws_bytes - 1, st), "short workspace")
    except RuntimeError as e:
        assert "code -3" in str(e), e
    else:
        raise AssertionError("short workspace: must be refused")
    assert not out.cpu().any() and not sizes.cpu().any()  # nothing was launched
    assert L.hf_png_bound(h, w, 2) == 0 and L.hf_png_segment_rows(0, w, c) == 0 and L.hf_png_workspace_bytes(0, h, w, c) == 0
    for exc, call in [(TypeError, lambda: M.png_encode(L, st, img.view(1, h, w, c).float())),
                      (ValueError, lambda: M.png_encode(L, st, img.view(h, w, c))),
                      (ValueError, lambda: M.png_encode(L, st, img[:h * w * 2].view(1, h, w, 2))),
                      (ValueError, lambda: M.png_encode(L, st, img.view(1, h, w, c), 4))]:
        try:
            call()
        except exc:
            pass
        else:
            raise AssertionError(f"expected {exc.__name__}")


def check_marshalled(L, st, device):
    """M.png_encode: the same bytes as the guarded call."""
    imgs = np.stack([smooth((9, 21, 3), k) for k in range(2)])
    files, sizes = M.png_encode(L, st, torch.from_numpy(imgs).to(device), 3)
    files, sizes = files.cpu().numpy(), sizes.cpu().numpy()
    assert [files[k, :sizes[k]].tobytes() for k in range(2)] == encode(L, st, device, imgs, 3)
