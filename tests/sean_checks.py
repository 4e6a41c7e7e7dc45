"""TEST INFRASTRUCTURE - direct checks of SEAN's table kernels (csrc/sean.hip: hf_label_conv3x3_f32, hf_ace_modulate_f32,
hf_ace_modulate_table_f32), shared by the hipsim tests (tests/test_sim_sean.py) and the GPU tests (tests/test_gpu_sean.py).
Built like tests/generator_ops_checks.py: every check takes (lib, st, dev, case); the rules of tests/small_ops_checks.py are
imported, not copied (region_mean and tanh of the same file are checked there).

Label conv.  Reference: the dense 3x3 convolution of the one-hot label map in torch fp64, weights = the sample's table columns.
A result is bias + at most nine table entries added in fp32 in some order - ten terms, (n - 1) * u * sum |terms| -, so with
A = |bias| + sum_tap |T|, per element:   |y - ref64| <= 9 * 2^-24 * A.
The two orders the kernels use - taps 0..8 onto the bias (general path), bias + (((t0 + t1) + ...) + t8) (interior path: one
lookup of the tap sum) - are restated in torch fp32, and which pixels take which is restated from the kernels' rules (per-pixel
kernel: a wave whose 64 pixels all have a one-label 3x3 neighbourhood inside the image, and only with the tap-sum scratch, i.e.
from 1024 pixels; four-pixel LDS kernel: per pixel): every output is predicted bit for bit.

ACE tail.  Reference: ACE.forward's tail (noise, inference BatchNorm, gamma / beta blend, (1 + gamma) * x + beta, LeakyReLU) in
fp64, the avg planes of the table form from the table in fp64; rule: small_ops_checks.accuracy against the same formula in ATen
fp32.  Exactness: table form == label conv + tail; x_up == the materialised nearest x2; batch rule; sentinels."""
import torch
import torch.nn.functional as F

from hairfastgan_amd import _marshal as M
from tests.small_ops_checks import ROWS, Case, _c, _guard_ok, _guarded, _sync, accuracy, exact, invariant  # noqa: F401

LABEL_TERMS = 10                         # bias + nine taps
LABEL_BOUND = (LABEL_TERMS - 1) * 2.0 ** -24
NL = 19                                  # SEAN's labels


# --------------------------------------------------------------------------------------------------------------------
# label conv
# --------------------------------------------------------------------------------------------------------------------
def label_inputs(seed, nb, H, W, C, nl, per_sample, group, band):
    """labels int32 [nb, H, W] in [0, nl): random, on planes of 1024 pixels or more the right half in 4 x 4 blocks (interiors of
    2 x 2 pixels); band: rows 7..13 of every map wholly label 7; table [9C, cols] with a DC offset (cols = batch * nl when every
    sample has its own columns, else nl), bias [C]."""
    torch.manual_seed(seed)
    labels = torch.randint(0, nl, (nb, H, W), dtype=torch.int32)
    if H * W >= 1024:
        blocks = torch.randint(0, nl, (nb, (H + 3) // 4, (W + 3) // 4), dtype=torch.int32).repeat_interleave(4, 1).repeat_interleave(4, 2)
        labels[:, :, W // 2:] = blocks[:, :H, W // 2:W]
    if band:
        labels[:, 7:14] = 7
    batch = nb * group
    table = torch.randn(9 * C, batch * nl if per_sample else nl) + 0.5
    return labels, table, torch.randn(C), batch


def dense_weights(table, C, col0, nl):
    """The table columns col0 .. col0 + nl as conv weights [C, nl, 3, 3] (table row = tap * C + channel)."""
    return table[:, col0:col0 + nl].reshape(3, 3, C, nl).permute(2, 3, 0, 1)


def label_restated(labels, table, bias, C, batch, nl, per_sample, group, relu):
    """(dense conv of the clamped one-hot map, A) in table's dtype, [batch, C, H, W]."""
    ys, As = [], []
    for b in range(batch):
        onehot = F.one_hot(labels[b // group].long().clamp(0, nl - 1), nl).permute(2, 0, 1)[None].to(table.dtype)
        w = dense_weights(table, C, b * nl if per_sample else 0, nl)
        ys.append(F.conv2d(onehot, w, bias, padding=1))
        As.append(F.conv2d(onehot, w.abs(), bias.abs(), padding=1))
    y = torch.cat(ys)
    return (F.relu(y) if relu else y), torch.cat(As)


def label_orders(lab, T, bias):
    """lab [H, W] clamped labels, T [9, C, nl] fp32 -> (general-path values, interior-path values [C, H, W] in fp32 in the
    kernels' orders, interior [H, W]: the 3x3 neighbourhood lies inside the image and carries one label)."""
    H, W = lab.shape
    C = T.shape[1]
    pad = F.pad(lab.long(), (1, 1, 1, 1), value=-1)
    acc = bias[:, None, None].expand(C, H, W).clone()
    interior = torch.ones(H, W, dtype=torch.bool)
    for t in range(9):
        l = pad[t // 3:t // 3 + H, t % 3:t % 3 + W]
        acc = torch.where(l >= 0, acc + T[t][:, l.clamp(min=0)], acc)
        interior &= l == lab
    ts = T[0]
    for t in range(1, 9):
        ts = ts + T[t]
    return acc, bias[:, None, None] + ts[:, lab.long()], interior


def label_predicted(labels, table, bias, C, batch, nl, per_sample, group, relu, kernel):
    """Every output's bits and the map of the pixels on the interior path, [batch, H, W]."""
    nb, H, W = labels.shape
    hw = H * W
    outs, paths = [], []
    for b in range(batch):
        col0 = b * nl if per_sample else 0
        T = table[:, col0:col0 + nl].reshape(9, C, nl)
        tap, tsum, interior = label_orders(labels[b // group].clamp(0, nl - 1), T, bias)
        if hw < 1024:
            interior = torch.zeros_like(interior)
        elif kernel == "pixel":  # the wave vote: lanes past the plane's end sit on its last pixel, a corner
            lanes = F.pad(interior.reshape(-1), (0, -hw % 64), value=False).reshape(-1, 64)
            interior = lanes.all(1, keepdim=True).expand(-1, 64).reshape(-1)[:hw].reshape(H, W)
        y = torch.where(interior, tsum, tap)
        outs.append(F.relu(y) if relu else y)
        paths.append(interior)
    return torch.stack(outs), torch.stack(paths)


def label_accuracy(op, label, got, ref64, A, t32):
    """|got - ref64| <= 9 * 2^-24 * A per element; the row holds the worst element's E_k and bound, and ATen fp32's E_t (not used)."""
    _sync(got.device)
    got = got.detach().cpu()
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all()), (op, label)
    err, bounds = (got.double() - ref64).abs(), LABEL_BOUND * A
    i = int(torch.argmax(err / bounds))
    e_k, bound, e_t = float(err.reshape(-1)[i]), float(bounds.reshape(-1)[i]), float((t32.double() - ref64).abs().max())
    ROWS.append((op, label, e_k, e_t, bound))
    print(f"sean {op} {label}: E_k {e_k:.2e} E_t {e_t:.2e} bound {bound:.2e} (E_k / (2^-24 A) {e_k / bound * (LABEL_TERMS - 1):.2f})")
    assert bool((err <= bounds).all()), (op, label, e_k, bound)


def _label_call(lib, st, dev, labels, table, bias, C, batch, nl, per_sample, group, relu):
    """The raw call into a guarded buffer, as M.label_conv3x3 makes it."""
    nb, H, W = labels.shape
    n = batch * C * H * W
    buf = _guarded(n, dev)
    tsum = table.new_empty((C, table.shape[1])) if H * W >= 1024 else None
    rc = lib.hf_label_conv3x3_f32(buf.data_ptr(), labels.data_ptr(), table.data_ptr(), bias.data_ptr(), batch, C, H, W, table.shape[1],
                                  nl if per_sample else 0, group, 1 if relu else 0, None if tsum is None else tsum.data_ptr(), st)
    _sync(dev)
    return buf, buf[:n].view(batch, C, H, W), rc


def check_label_conv(lib, st, dev, case):
    nb, H, W, C, nl, per_sample, group, relu, kernel, band = case.args
    assert (kernel == "v4") == (H * W >= 1024 and W % 4 == 0 and nl <= 32), case.label  # the launcher's rule, as the case states it
    labels, table, bias, batch = label_inputs(400, nb, H, W, C, nl, per_sample, group, band)
    args = (C, batch, nl, per_sample, group, relu)
    ld, td, bd = labels.to(dev), table.to(dev), bias.to(dev)
    y = M.label_conv3x3(lib, st, ld, td, bd, C, batch=batch, cols_per_sample=nl if per_sample else 0, group=group, relu=relu)
    ref64, A = label_restated(labels, table.double(), bias.double(), *args)
    label_accuracy("label_conv", case.label, y, ref64, A, label_restated(labels, table, bias, *args)[0])
    buf, raw, rc = _label_call(lib, st, dev, ld, td, bd, *args)
    _guard_ok("label_conv", case.label, buf, raw.numel(), rc)
    exact("label_conv", case.label + " raw call", raw, y.cpu())
    want, path = label_predicted(labels, table, bias, *args, kernel)
    exact("label_conv", case.label + " predicted bits", y, want)
    print(f"sean label_conv {case.label}: {int(path.sum())} of {path.numel()} pixels on the tap-sum path")
    if band:
        # row 10: its neighbours are rows 9..11 of the band.  Per-pixel kernel: the one wave inside the row's interior, pixels
        # 10 W + 4 .. 10 W + 67 (W = 70: pixels 704..767), votes for the tap sum, the pixels next to it take the taps in order;
        # four-pixel kernel: every interior pixel takes the tap sum, the two border pixels the taps
        T = table[:, :nl].reshape(9, C, nl)
        tap, tsum, _ = label_orders(labels[0], T, bias)
        assert bool((tap[:, 10, 1:W - 1] != tsum[:, 10, 1:W - 1]).any(0).all()), "the two orders must differ for this seed"
        got = y.cpu()[0]
        lo = ((-10 * W) % 64 or 64) if kernel == "pixel" else 1
        hi = lo + 64 if kernel == "pixel" else W - 1
        assert kernel == "v4" or (hi <= W - 1 and (10 * W + lo) % 64 == 0)
        assert hi - lo >= 64 and bool(path[0, 10, lo:hi].all()) and torch.equal(got[:, 10, lo:hi], tsum[:, 10, lo:hi])
        rest = [x for x in range(W) if not lo <= x < hi]
        assert rest and not bool(path[0, 10, rest].any()) and torch.equal(got[:, 10, rest], tap[:, 10, rest])


def check_label_clamp(lib, st, dev, case):
    """Labels 255, -3 and 19 give the clamped map's bits."""
    (H, W) = case.args
    labels, table, bias, _ = label_inputs(401, 1, H, W, 6, NL, False, 1, False)
    labels[0, 2, 3], labels[0, 4, 4], labels[0, 0, 0] = 255, -3, 19
    td, bd = table.to(dev), bias.to(dev)
    want = M.label_conv3x3(lib, st, labels.clamp(0, NL - 1).to(dev), td, bd, 6)
    exact("label_clamp", case.label, M.label_conv3x3(lib, st, labels.to(dev), td, bd, 6), want.cpu())
    ref64, A = label_restated(labels, table.double(), bias.double(), 6, 1, NL, False, 1, False)
    label_accuracy("label_clamp", case.label, want, ref64, A, label_restated(labels, table, bias, 6, 1, NL, False, 1, False)[0])


def check_label_forms(lib, st, dev, case):
    """One map through both kernels - the per-pixel one reached with a table of 40 columns of which the map uses 19 -: each
    inside the fp64 bound, so within twice the bound of each other."""
    H, W, C = case.args
    labels, table, bias, _ = label_inputs(402, 1, H, W, C, NL, False, 1, False)
    torch.manual_seed(403)
    wide = torch.cat([table, torch.randn(9 * C, 40 - NL)], 1).contiguous()
    ld, bd = labels.to(dev), bias.to(dev)
    v4 = M.label_conv3x3(lib, st, ld, table.to(dev), bd, C)
    px = M.label_conv3x3(lib, st, ld, wide.to(dev), bd, C)
    ref64, A = label_restated(labels, table.double(), bias.double(), C, 1, NL, False, 1, False)
    t32 = label_restated(labels, table, bias, C, 1, NL, False, 1, False)[0]
    label_accuracy("label_forms", case.label + " four-pixel kernel", v4, ref64, A, t32)
    label_accuracy("label_forms", case.label + " per-pixel kernel", px, ref64, A, t32)
    exact("label_forms", case.label + " four-pixel kernel, predicted bits", v4, label_predicted(labels, table, bias, C, 1, NL, False, 1, False, "v4")[0])
    exact("label_forms", case.label + " per-pixel kernel, predicted bits", px, label_predicted(labels, wide, bias, C, 1, 40, False, 1, False, "pixel")[0])
    assert bool(((v4.cpu().double() - px.cpu().double()).abs() <= 2 * LABEL_BOUND * A).all())


# --------------------------------------------------------------------------------------------------------------------
# ACE tail
# --------------------------------------------------------------------------------------------------------------------
def up2(x):
    return x.repeat_interleave(2, 2).repeat_interleave(2, 3).contiguous()


def ace_restated(x, r, nv, sc, sh, avg, sp, blend, group, slope):
    """ACE.forward's tail in x's dtype; r [B, H, W] | None, avg [B, 2C, H, W] | None, sp [B / group, 2C, H, W]."""
    C = x.shape[1]
    cv = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    n = (x if r is None else x + r[:, None] * cv(nv)) * cv(sc) + cv(sh)
    spx = sp.repeat_interleave(group, 0)
    g, bt = spx[:, :C], spx[:, C:]
    if avg is not None:
        ag, ab = torch.sigmoid(blend[0]), torch.sigmoid(blend[1])
        g, bt = ag * avg[:, :C] + (1 - ag) * g, ab * avg[:, C:] + (1 - ab) * bt
    return F.leaky_relu(n * (1 + g) + bt, slope)


def ace_inputs(seed, B, C, H, W, group, noise, x_up=False):
    torch.manual_seed(seed)
    t = {"x": torch.randn(B, C, H // 2, W // 2) if x_up else torch.randn(B, C, H, W), "r": torch.randn(B, H, W) if noise else None,
         "nv": torch.randn(C) * 0.1 if noise else None, "sc": torch.rand(C) + 0.5, "sh": torch.randn(C),
         "sp": torch.randn(B // group, 2 * C, H, W), "blend": torch.tensor([0.3, -0.7])}
    return t


def _to(t, f):
    return {k: (None if v is None else f(v)) for k, v in t.items()}


def _blocky(seed, nb, H, W):
    """Label maps with interiors, borders and single pixels: 4 x 4 blocks, a random quarter of the plane, one stray label."""
    torch.manual_seed(seed)
    lab = torch.randint(0, NL, (nb, (H + 3) // 4, (W + 3) // 4), dtype=torch.int32).repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W]
    lab = lab.contiguous()
    lab[:, :H // 2, :W // 2] = torch.randint(0, NL, (nb, H // 2, W // 2), dtype=torch.int32)
    lab[:, H - 3, W - 3] = 11
    return lab


def check_ace(lib, st, dev, case):
    """The two-kernel form: avg is an input."""
    B, C, H, W, group, noise, with_avg, slope, x_up = case.args
    t = ace_inputs(410, B, C, H, W, group, noise, x_up)
    avg = torch.randn(B, 2 * C, H, W) if with_avg else None
    blend = t["blend"] if with_avg else None
    d = _to(t, lambda v: v.to(dev))
    avg_d = None if avg is None else avg.to(dev)
    run = lambda x, up: M.ace_modulate(lib, st, x, d["r"], d["nv"], d["sc"], d["sh"], avg_d, d["sp"], None if blend is None else d["blend"],  # noqa: E731
                                       group=group, slope=slope, x_up=up)
    got = run(d["x"], x_up)
    x_full = up2(t["x"]) if x_up else t["x"]
    t64 = _to(t, lambda v: v.double())
    ref = ace_restated(x_full.double(), t64["r"], t64["nv"], t64["sc"], t64["sh"], None if avg is None else avg.double(), t64["sp"], t64["blend"],
                       group, slope)
    accuracy("ace", case.label, got, ref, ace_restated(x_full, t["r"], t["nv"], t["sc"], t["sh"], avg, t["sp"], t["blend"], group, slope), tag="sean")
    if x_up:
        exact("ace", case.label + " == materialised x2", got, run(x_full.to(dev), False).cpu())
    n = B * C * H * W
    buf = _guarded(n, dev)
    p = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    rc = lib.hf_ace_modulate_f32(buf.data_ptr(), d["x"].data_ptr(), p(d["r"]), p(d["nv"]), d["sc"].data_ptr(), d["sh"].data_ptr(), p(avg_d),
                                 d["sp"].data_ptr(), None if blend is None else d["blend"].data_ptr(), B, C, H * W, group, float(slope),
                                 W if x_up else 0, st)
    _guard_ok("ace", case.label, buf, n, rc)
    exact("ace", case.label + " raw call", buf[:n].view(B, C, H, W), got.cpu())


def check_ace_table(lib, st, dev, case):
    """The table form: the avg planes are formed in the kernel; the reference forms them in fp64 from the table."""
    nb, group, C, H, W, noise, x_up = case.args
    B = nb * group
    t = ace_inputs(411, B, C, H, W, group, noise, x_up)
    labels = _blocky(412, nb, H, W)
    torch.manual_seed(413)
    table, avg_bias = torch.randn(9 * 2 * C, B * NL) + 0.5, torch.randn(2 * C)
    d = _to(t, lambda v: v.to(dev))
    ld, td, abd = labels.to(dev), table.to(dev), avg_bias.to(dev)
    run = lambda x, up: M.ace_modulate_table(lib, st, x, d["r"], d["nv"], d["sc"], d["sh"], ld, td, abd, d["sp"], d["blend"], group=group,  # noqa: E731
                                             slope=0.2, x_up=up)
    got = run(d["x"], x_up)
    x_full = up2(t["x"]) if x_up else t["x"]
    t64 = _to(t, lambda v: v.double())
    avg64 = label_restated(labels, table.double(), avg_bias.double(), 2 * C, B, NL, True, group, False)[0]
    avg32 = label_restated(labels, table, avg_bias, 2 * C, B, NL, True, group, False)[0]
    ref = ace_restated(x_full.double(), t64["r"], t64["nv"], t64["sc"], t64["sh"], avg64, t64["sp"], t64["blend"], group, 0.2)
    accuracy("ace_table", case.label, got, ref, ace_restated(x_full, t["r"], t["nv"], t["sc"], t["sh"], avg32, t["sp"], t["blend"], group, 0.2),
             tag="sean")
    avg_k = M.label_conv3x3(lib, st, ld, td, abd, 2 * C, batch=B, cols_per_sample=NL, group=group)
    two = M.ace_modulate(lib, st, d["x"], d["r"], d["nv"], d["sc"], d["sh"], avg_k, d["sp"], d["blend"], group=group, slope=0.2, x_up=x_up)
    exact("ace_table", case.label + " == label conv + tail", got, two.cpu())
    if x_up:
        exact("ace_table", case.label + " == materialised x2", got, run(x_full.to(dev), False).cpu())
    n = B * C * H * W
    buf = _guarded(n, dev)
    p = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    rc = lib.hf_ace_modulate_table_f32(buf.data_ptr(), d["x"].data_ptr(), p(d["r"]), p(d["nv"]), d["sc"].data_ptr(), d["sh"].data_ptr(),
                                       ld.data_ptr(), td.data_ptr(), abd.data_ptr(), d["sp"].data_ptr(), d["blend"].data_ptr(), B, C, H, W,
                                       table.shape[1], NL, group, 0.2, 1 if H * W >= 1024 else 0, 1 if x_up else 0, st)
    _guard_ok("ace_table", case.label, buf, n, rc)
    exact("ace_table", case.label + " raw call", buf[:n].view(B, C, H, W), got.cpu())


# --------------------------------------------------------------------------------------------------------------------
# the case tables: the smallest shapes that reach each branch (size classes as in small_ops_checks)
# --------------------------------------------------------------------------------------------------------------------
CASES = {
    # (label maps, H, W, C, labels, own columns per sample, group, ReLU, kernel, band of one label)
    "label_conv": [
        _c("2x9x12 C6 ReLU: per-pixel kernel, small plane", 2, 9, 12, 6, NL, False, 1, True, "pixel", False),
        _c("2x9x12 C8 group 2, own columns", 2, 9, 12, 8, NL, True, 2, False, "pixel", False),
        _c("1x16x70 C5 band: per-pixel kernel with the tap-sum scratch, one wave votes", 1, 16, 70, 5, NL, False, 1, False, "pixel", True),
        _c("1x16x70 C5 band, 40 labels", 1, 16, 70, 5, 40, False, 1, False, "pixel", True),
        _c("2x32x40 C70 group 2 ReLU: four-pixel kernel, ragged channel chunk", 2, 32, 40, 70, NL, True, 2, True, "v4", False),
        _c("1x32x32 C3 group 3: exactly 1024 pixels", 1, 32, 32, 3, NL, True, 3, False, "v4", False),
        _c("1x40x28 C4, 32 labels", 1, 40, 28, 4, 32, False, 1, False, "v4", False),
        _c("1x16x72 C5 band: four-pixel kernel", 1, 16, 72, 5, NL, False, 1, False, "v4", True),
    ],
    "label_clamp": [_c("9x12 per-pixel kernel", 9, 12), _c("32x40 four-pixel kernel", 32, 40)],
    "label_forms": [_c("32x40 C6", 32, 40, 6)],
    # (B, C, H, W, group, noise, avg, slope, x_up)
    "ace": [
        _c("4x4x9x12 group 2, noise, avg", 4, 4, 9, 12, 2, True, True, 0.2, False),
        _c("4x4x9x12 group 2, no noise, no avg, slope 1", 4, 4, 9, 12, 2, False, False, 1.0, False),
        _c("4x5x32x40 group 2, x_up", 4, 5, 32, 40, 2, True, True, 0.2, True),
        _c("4x5x32x40 group 2, x_up, no noise, no avg, slope 1", 4, 5, 32, 40, 2, False, False, 1.0, True),
    ],
    # (label maps, group, C, H, W, noise, x_up)
    "ace_table": [
        _c("2 maps, group 2, C37, 32x40: ragged channel chunk", 2, 2, 37, 32, 40, True, False),
        _c("1 map, group 3, C6, 34x36, x_up, no noise", 1, 3, 6, 34, 36, False, True),
    ],
}
CHECKS = {op: globals()["check_" + op] for op in CASES}


def cases(gpu):
    return [(op, c) for op, cs in CASES.items() for c in cs if gpu or c.size < 2]


def case_id(v):
    return v.label.replace(" ", "_") if isinstance(v, Case) else str(v)


# --------------------------------------------------------------------------------------------------------------------
# batch invariance of both tails (and of the label conv under the table form): run(n) = the first n samples, group 1
# --------------------------------------------------------------------------------------------------------------------
def _batch_runs(lib, st, dev):
    g = {}
    nb = 9
    t = _to(ace_inputs(430, nb, 4, 9, 12, 1, True), lambda v: v.to(dev))
    torch.manual_seed(431)
    avg = torch.randn(nb, 8, 9, 12).to(dev)
    g["ace"] = lambda n: M.ace_modulate(lib, st, t["x"][:n], t["r"][:n], t["nv"], t["sc"], t["sh"], avg[:n], t["sp"][:n], t["blend"], slope=0.2)
    u = _to(ace_inputs(432, nb, 3, 32, 40, 1, True), lambda v: v.to(dev))
    labels = _blocky(433, nb, 32, 40).to(dev)
    table, avg_bias = (torch.randn(9 * 6, nb * NL) + 0.5).to(dev), torch.randn(6).to(dev)
    g["ace_table"] = lambda n: M.ace_modulate_table(lib, st, u["x"][:n], u["r"][:n], u["nv"], u["sc"], u["sh"], labels[:n].contiguous(), table,
                                                    avg_bias, u["sp"][:n], u["blend"], slope=0.2)
    g["label_conv"] = lambda n: M.label_conv3x3(lib, st, labels[:n].contiguous(), table, avg_bias, 6, batch=n, cols_per_sample=NL)
    return g


BATCH_OPS = ["ace", "ace_table", "label_conv"]


def check_batch_invariance(lib, st, dev, op):
    invariant(op, _batch_runs(lib, st, dev)[op])
