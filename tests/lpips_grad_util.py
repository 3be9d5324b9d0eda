"""Yardsticks and checks of the LPIPS input gradient (csrc/lpips.hip, include/dgs_lpips.h 'The input gradient', dgs_amd.lpips), in the
pattern of tests/lpips_util.py, whose weights, images and restatement are used here.  Every check is a function of a device:
tests/test_lpips_grad_emu.py runs it on the CPU-emulated build of the kernels, tests/test_lpips_grad_gpu.py on the GPU.

Bars.
  conv data gradient  exact: integer data (dy in [-2, 2], w in [-1, 1], integer mask and add) whose partial sums stay below 2^24,
                      compared bit for bit with fp64 F.conv_transpose2d(dy, w, padding=1) and the rule (mask > 0 ? . : 0) + add
  pool backward       exact: x integer in [-1, 1] (ties everywhere), against a numpy restatement of the first-maximum rule and
                      against torch's CPU autograd of F.max_pool2d on the same data
  tap backward        exactly 0 where f is 0 and for f0 == f1; elsewhere per pair: relative L2 against fp64 autograd (through relu)
                      <= FEATURE_FACTOR (8) x that of the same formula in fp32 torch autograd on the CPU
  whole network       gradient of out.sum() with respect to both inputs, per image: relative L2 against fp64 autograd of
                      lpips_util.restatement_impl <= 8 x that of the fp32 restatement's autograd on the same case (measured on the CPU
                      with reference forms only: the fp32 restatement lies at 1.5e-6 to 2.6e-6 on the five NET_CASES, a second,
                      32-blocked fp32 order at 0.79 to 1.28 x of it; no pixel vector of any tap is all zero there, so no NaN)
"""
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

import lpips_util as LU
from lpips_util import P, _native, _guarded, _guards_intact, _ptr, _stream, lib_of, model, rel_l2, same_bytes  # noqa: F401

FEATURE_FACTOR = LU.FEATURE_FACTOR
INVALID = -1                                       # DGS_ERR_INVALID_ARGUMENT

CONV_GRAD_CASES = [  # N, H, W, channels of dy, channels of dx
    (1, 1, 1, 64, 64),
    (2, 3, 5, 64, 3),         # the first layer
    (1, 7, 9, 128, 64),
    (3, 5, 4, 256, 128),
    (2, 9, 15, 512, 256),
    (1, 16, 16, 512, 512),
    (1, 6, 7, 72, 32),        # the scalar staging path
    (2, 5, 6, 136, 5),
    (1, 19, 14, 64, 64),
]
POOL_GRAD_CASES = [(2, 2), (3, 5), (35, 21), (16, 16), (1, 4)]
TAP_CASES = LU.TAP_CASES
NET_CASES = LU.NET_CASES


def check_conv_grad_exact(device, N, H, W, Cdy, Cdx, epilogue):
    L = lib_of(device)
    g = torch.Generator().manual_seed(N * 1000 + H * 100 + W * 10 + Cdy + Cdx + 7)
    dy = torch.randint(-2, 3, (N, Cdy, H, W), generator=g).float()
    w = torch.randint(-1, 2, (Cdy, Cdx, 3, 3), generator=g).float()        # the forward's weight [Cout, Cin, 3, 3]
    mask = torch.randint(-2, 3, (N, Cdx, H, W), generator=g).float()
    add = torch.randint(-3, 4, (N, Cdx, H, W), generator=g).float()
    want = F.conv_transpose2d(dy.double(), w.double(), padding=1)
    assert float(want.abs().max()) < 2 ** 24 - 4
    if epilogue:
        want = torch.where(mask.double() > 0, want, torch.zeros_like(want)) + add.double()
    last = lambda t: t.permute(0, 2, 3, 1).contiguous().to(device)
    dyd, maskd, addd = last(dy), last(mask), last(add)
    packed = P.pack_weights_transposed(w.to(device), L)
    assert packed.numel() == ((9 * Cdy + 31) // 32 * 32) * ((Cdx + 63) // 64 * 64)
    buf, dx = _guarded(N * H * W * Cdx, device)
    a = _native.DgsConv3x3BackwardDataArgs(N, H, W, Cdx, Cdy, _ptr(dyd), _ptr(packed), _ptr(maskd) if epilogue else None,
                                           _ptr(addd) if epilogue else None, _ptr(dx))
    assert L.dgs_conv3x3_backward_data(ctypes.byref(a), _stream(dyd)) == 0
    got = dx.reshape(N, H, W, Cdx).permute(0, 3, 1, 2).cpu()
    assert _guards_intact(buf.cpu()), "dgs_conv3x3_backward_data wrote outside its output"
    assert torch.equal(got.double(), want), f"max abs difference {float((got.double() - want).abs().max())}"
    wrapped = P.conv3x3_backward_data(dyd, packed, Cdx, maskd if epilogue else None, addd if epilogue else None, L)
    assert torch.equal(wrapped.cpu(), dx.reshape(N, H, W, Cdx).cpu())
    if epilogue:                                   # add may be the output itself
        inplace = addd.clone()
        a = _native.DgsConv3x3BackwardDataArgs(N, H, W, Cdx, Cdy, _ptr(dyd), _ptr(packed), _ptr(maskd), _ptr(inplace), _ptr(inplace))
        assert L.dgs_conv3x3_backward_data(ctypes.byref(a), _stream(dyd)) == 0
        assert torch.equal(inplace.cpu(), wrapped.cpu())
    # the transposed operand is the plain operand of the flipped, transposed tensor
    assert torch.equal(packed.cpu(), P.pack_weights(w.flip(2, 3).transpose(0, 1).contiguous().to(device), L).cpu())


def pool_backward_restatement(x, dy, relu_mask, add):
    """numpy, NCHW: dy goes to the first maximum of its window in (row, column) order (`>` against the running maximum)."""
    N, C, H, W = x.shape
    dx = np.zeros_like(x)
    for ho in range(H // 2):
        for wo in range(W // 2):
            best = x[:, :, 2 * ho, 2 * wo].copy()
            at = np.zeros(best.shape, dtype=np.int64)
            for k, (i, j) in enumerate(((0, 1), (1, 0), (1, 1)), start=1):
                v = x[:, :, 2 * ho + i, 2 * wo + j]
                better = v > best
                best = np.where(better, v, best)
                at = np.where(better, k, at)
            for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                dx[:, :, 2 * ho + i, 2 * wo + j] = np.where(at == k, dy[:, :, ho, wo], np.float32(0))
    if relu_mask:
        dx = np.where(x > 0, dx, np.float32(0))
    if add is not None:
        dx = dx + add
    return dx.astype(np.float32)


def check_pool_backward_exact(device, H, W):
    L = lib_of(device)
    N, C = 2, 7
    g = torch.Generator().manual_seed(H * 100 + W + 3)
    x = torch.randint(-1, 2, (N, C, H, W), generator=g).float()
    dy = torch.randn(N, C, H // 2, W // 2, generator=g)
    add = torch.randn(N, C, H, W, generator=g)
    last = lambda t: t.permute(0, 2, 3, 1).contiguous().to(device)
    xd, dyd, addd = last(x), last(dy), last(add)
    for relu_mask, use_add in ((0, False), (1, True), (0, True), (1, False)):
        want = torch.from_numpy(pool_backward_restatement(x.numpy(), dy.numpy(), relu_mask, add.numpy() if use_add else None))
        buf, dx = _guarded(x.numel(), device)
        a = _native.DgsMaxPool2x2BackwardArgs(N, H, W, C, _ptr(xd), _ptr(dyd) if dy.numel() else None, relu_mask, _ptr(addd) if use_add else None,
                                              _ptr(dx))
        assert L.dgs_maxpool2x2_backward(ctypes.byref(a), _stream(xd)) == 0
        got = dx.reshape(N, H, W, C).permute(0, 3, 1, 2).cpu()
        assert _guards_intact(buf.cpu()), "dgs_maxpool2x2_backward wrote outside its output"
        assert same_bytes(got, want), (relu_mask, use_add)
        if dy.numel():
            assert same_bytes(P.maxpool2x2_backward(xd, dyd, bool(relu_mask), addd if use_add else None, L).cpu(), dx.reshape(N, H, W, C).cpu())
        if use_add:                                # add may be the output itself
            inplace = addd.clone()
            a = _native.DgsMaxPool2x2BackwardArgs(N, H, W, C, _ptr(xd), _ptr(dyd) if dy.numel() else None, relu_mask, _ptr(inplace), _ptr(inplace))
            assert L.dgs_maxpool2x2_backward(ctypes.byref(a), _stream(xd)) == 0
            assert same_bytes(inplace.reshape(N, H, W, C).permute(0, 3, 1, 2).cpu(), want)
        if not relu_mask and not use_add:
            if H > 1 and W > 1:                    # torch's own routing on the same ties
                leaf = x.clone().requires_grad_(True)
                F.max_pool2d(leaf, 2, 2).backward(dy)
                assert same_bytes(got, leaf.grad)
            else:
                assert bool((got == 0).all())


def tap_inputs(N, H, W, C):
    """The features of lpips_util.check_tap, with their three all-zero pixel vectors."""
    g = torch.Generator().manual_seed(N + H * 7 + W * 13 + C)
    f0 = F.relu(torch.randn(N, H, W, C, generator=g) - 0.3)
    f1 = F.relu(f0 + 0.5 * torch.randn(N, H, W, C, generator=g))
    flat0, flat1 = f0.view(-1, C), f1.view(-1, C)
    flat0[0] = 0
    if flat0.shape[0] > 1:
        flat1[1] = 0
    if flat0.shape[0] > 2:
        flat0[2] = 0
        flat1[2] = 0
    lin = torch.rand(C, generator=g) * 0.1
    return f0, f1, lin


def tap_autograd(f0, f1, lin, dtype):
    """The gradient of sum_n d[n] with respect to the ReLU's inputs, by torch autograd in `dtype` on the CPU."""
    z0, z1 = f0.detach().clone().to(dtype).requires_grad_(True), f1.detach().clone().to(dtype).requires_grad_(True)
    a, b = F.relu(z0), F.relu(z1)
    h0 = a / (a.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    h1 = b / (b.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    ((h0 - h1) ** 2 * lin.to(dtype)).sum(-1).mean(dim=(1, 2)).sum().backward()
    return z0.grad, z1.grad


def check_tap_backward(device, N, H, W, C):
    """-> rows (what, measured / bar)."""
    L = lib_of(device)
    f0, f1, lin = tap_inputs(N, H, W, C)
    w0, w1 = tap_autograd(f0, f1, lin, torch.float64)
    s0, s1 = tap_autograd(f0, f1, lin, torch.float32)
    assert bool(torch.isfinite(w0).all() and torch.isfinite(w1).all() and torch.isfinite(s0).all() and torch.isfinite(s1).all())
    d0, d1, dl = f0.to(device), f1.to(device), lin.to(device)
    g0, g1 = (t.cpu() for t in P.tap_backward(d0, d1, dl, True, L))
    a0, a1 = (t.cpu() for t in P.tap_backward(d0, d1, dl, True, L))
    assert same_bytes(g0, a0) and same_bytes(g1, a1)
    only0, none = P.tap_backward(d0, d1, dl, False, L)
    assert none is None and same_bytes(only0.cpu(), g0)
    assert bool((g0[f0 == 0] == 0).all()) and bool((g1[f1 == 0] == 0).all())
    z0, z1 = P.tap_backward(d0, d0, dl, True, L)
    assert bool((z0.cpu() == 0).all()) and bool((z1.cpu() == 0).all())
    rows = []
    for n in range(N):
        for name, got, want, single in (("g0", g0, w0, s0), ("g1", g1, w1, s1)):
            e, bar = rel_l2(got[n], want[n]), FEATURE_FACTOR * rel_l2(single[n], want[n])
            if float(want[n].abs().max()) == 0:
                assert bool((got[n] == 0).all())
                continue
            rows.append((f"tap backward N={N} H={H} W={W} C={C} pair{n} {name}", e / bar, e, bar))
    for what, ratio, e, bar in rows:
        print(f"{what}: measured / bar = {ratio:.4f}   ({e:.3e} against {bar:.3e})")
    assert all(r[1] <= 1.0 for r in rows), [r for r in rows if r[1] > 1.0]
    return rows


@functools.lru_cache(maxsize=None)
def net_grad_reference(n, h, w):
    """(g64_0, g64_1, g32_0, g32_1): autograd of the restatement's out.sum() in fp64 and in fp32, computed once and shared."""
    sd = LU.random_state_dict(0)
    x0, x1 = LU.net_reference(n, h, w)[:2]
    out = []
    for dtype in (torch.float64, torch.float32):
        a, b = x0.detach().clone().to(dtype).requires_grad_(True), x1.detach().clone().to(dtype).requires_grad_(True)
        LU.restatement_impl(sd, a, b, dtype, lambda t: t.to(dtype))[0].sum().backward()
        assert bool(torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all())
        out += [a.grad, b.grad]
    return tuple(out)


def check_network_grad(device, n, h, w):
    """-> rows (what, measured / bar, measured, yardstick's error) of the case, one per image."""
    x0, x1 = LU.net_reference(n, h, w)[:2]
    g64_0, g64_1, g32_0, g32_1 = net_grad_reference(n, h, w)
    m = grad_model(device)
    a, b = x0.detach().clone().to(device).requires_grad_(True), x1.detach().clone().to(device).requires_grad_(True)
    out = m(a, b)
    assert tuple(out.shape) == (n, 1, 1, 1) and out.grad_fn is not None
    assert same_bytes(out.detach().reshape(-1).cpu(), m.run(x0.to(device), x1.to(device))["out"].cpu())
    out.sum().backward()
    rows = []
    for name, got, g64, g32 in (("x0", a.grad.cpu(), g64_0, g32_0), ("x1", b.grad.cpu(), g64_1, g32_1)):
        for i in range(n):
            e, e32 = rel_l2(got[i], g64[i]), rel_l2(g32[i], g64[i])
            rows.append((f"d out / d {name}[{i}]", e / (FEATURE_FACTOR * e32), e, e32))
    for what, ratio, e, e32 in rows:
        print(f"network gradient n={n} {h}x{w} {what}: measured / bar = {ratio:.4f}   ({e:.3e}, fp32 restatement {e32:.3e})")
    assert all(r[1] <= 1.0 for r in rows), [r for r in rows if r[1] > 1.0]
    return rows


_grad_models = {}


def grad_model(device, seed=0):
    """lpips_util.model's weights in a module built with differentiable=True."""
    key = (str(device), seed)
    if key not in _grad_models:
        m = P.LPIPS(net="vgg", lib=lib_of(device) if str(device) == "cpu" else None, differentiable=True)
        m.load_state_dict(LU.random_state_dict(seed), strict=True)
        _grad_models[key] = m.to(device)
    return _grad_models[key]


PROPERTIES = ["repeat", "permute", "alone", "chunked", "without_grad1", "identical", "backward_scales"]
_base = {}


def _property_base(device, h=16, w=19):
    """Three pairs of 16 x 19 and their out, taps and gradients: computed once per device, shared and left unchanged."""
    if str(device) not in _base:
        x0, x1 = LU.images(3, h, w, seed=7)
        x0, x1 = x0.to(device), x1.to(device)
        _base[str(device)] = (x0, x1, grad_model(device).run_with_gradient(x0, x1, both=True, want_taps=True))
    return _base[str(device)]


def _same(r, out, taps, g0, g1, rows=slice(None)):
    ok = same_bytes(r["out"].cpu(), out[rows]) and same_bytes(r["grad0"].cpu(), g0[rows])
    if r["per_tap"] is not None:
        ok = ok and same_bytes(r["per_tap"].cpu(), taps[rows])
    if r["grad1"] is not None:
        ok = ok and same_bytes(r["grad1"].cpu(), g1[rows])
    return ok


def check_property(device, which, thorough=True):
    """One of PROPERTIES, bitwise.  thorough=False (the emulator, where one call on the three pairs takes ten seconds): 'alone' takes
    the middle pair only, 'chunked' chunks of 2 only, 'backward_scales' the call with both inputs only."""
    m = grad_model(device)
    x0, x1, base = _property_base(device)
    out, taps, g0, g1 = (base[k].cpu() for k in ("out", "per_tap", "grad0", "grad1"))
    assert bool((out > 0).all()) and float(g0.abs().max()) > 0 and float(g1.abs().max()) > 0
    assert same_bytes(out, m.run(x0, x1)["out"].cpu())                       # the forward's bytes
    run = lambda a, b, **kw: m.run_with_gradient(a, b, want_taps=True, **kw)
    if which == "repeat":
        assert _same(run(x0, x1), out, taps, g0, g1)
    elif which == "permute":
        perm = torch.tensor([2, 0, 1])
        assert _same(run(x0[perm.to(device)], x1[perm.to(device)]), out, taps, g0, g1, perm)
    elif which == "alone":
        for i in (range(3) if thorough else (1,)):
            assert _same(run(x0[i:i + 1], x1[i:i + 1]), out, taps, g0, g1, slice(i, i + 1))
    elif which == "chunked":
        for chunk in ((1, 2) if thorough else (2,)):
            assert _same(run(x0, x1, chunk=chunk), out, taps, g0, g1)
    elif which == "without_grad1":    # grad0 is the same bytes whether grad1 was asked for or not
        r = run(x0, x1, both=False)
        assert r["grad1"] is None and _same(r, out, taps, g0, g1)
        if thorough:
            r = run(x0, x1, both=False, chunk=2)
            assert _same(r, out, taps, g0, g1)
    elif which == "identical":        # the gradient of lpips(x, x) is all zeros
        r = run(x0, x0)
        assert bool((r["out"].cpu() == 0).all()) and bool((r["grad0"].cpu() == 0).all()) and bool((r["grad1"].cpu() == 0).all())
    elif which == "backward_scales":  # backward multiplies the stored rows by grad_out[n]; only an input that requires grad gets one
        a, b = x0.clone().requires_grad_(True), x1.clone().requires_grad_(True)
        o = m(a, b)
        scale = torch.tensor([2.0, 0.0, -1.0], device=o.device)
        o.reshape(-1).backward(scale)
        s = scale.cpu().reshape(-1, 1, 1, 1)
        assert same_bytes(a.grad.cpu(), s * g0) and same_bytes(b.grad.cpu(), s * g1)
        if not thorough:
            return
        a2 = x0.clone().requires_grad_(True)
        m(a2, x1).sum().backward()
        assert same_bytes(a2.grad.cpu(), g0)
        b2 = x1.clone().requires_grad_(True)
        m(x0, b2).sum().backward()                 # the second input alone: the library sees the pair swapped
        assert rel_l2(b2.grad.cpu(), g1) < 1e-5
    else:
        raise ValueError(which)


def check_surface(device):
    L = lib_of(device)
    x0, x1 = LU.images(1, 16, 16, seed=5)
    x0, x1 = x0.to(device), x1.to(device)
    with torch.enable_grad():
        try:
            model(device)(x0.clone().requires_grad_(True), x1)            # the default module still refuses
            raise AssertionError("the default module accepted an input that requires grad")
        except NotImplementedError as e:
            assert "input gradient" in str(e)
    m = grad_model(device)
    want = model(device)(x0, x1)
    with torch.no_grad():
        y = m(x0.clone().requires_grad_(True), x1)
    assert y.grad_fn is None and not y.requires_grad and same_bytes(y.cpu(), want.cpu())
    y = m(x0, x1)                                                          # no input requires grad: the metric's path
    assert y.grad_fn is None and same_bytes(y.cpu(), want.cpu())
    a = x0.clone().requires_grad_(True)
    y = m(a, x1)
    assert same_bytes(y.detach().cpu(), want.cpu())
    s = torch.ones((), device=y.device, requires_grad=True)               # a grad_out that requires grad: a second derivative is asked for
    (g,) = torch.autograd.grad(y.sum() * s, a, create_graph=True)
    try:
        g.sum().backward()
        raise AssertionError("a second derivative was computed")
    except RuntimeError as e:
        assert "once_differentiable" in str(e), str(e)
    for bad in ((1, 15, 16), (1, 16, 15)):
        try:
            m(torch.zeros(*bad[:1], 3, *bad[1:], device=device).requires_grad_(True), torch.zeros(*bad[:1], 3, *bad[1:], device=device))
            raise AssertionError("an image below 16 x 16 was accepted")
        except ValueError as e:
            assert "16 x 16" in str(e)
    # the C ABI itself
    pk = m.packed(transposed=True)
    assert len(pk["conv_wt"]) == 13 and m.packed() is pk and m.packed(transposed=True) is pk
    n, h, w = 1, 16, 16
    nbytes = int(L.dgs_lpips_grad_workspace_bytes(n, h, w))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    out = torch.empty(n, dtype=torch.float32, device=device)
    grad0 = torch.empty(n, 3, h, w, dtype=torch.float32, device=device)

    def args(H=h, W=w, g0=grad0, bytes_=nbytes):
        a = _native.DgsLpipsGradArgs()
        a.N, a.H, a.W, a.x0, a.x1, a.shift, a.scale = n, H, W, _ptr(x0), _ptr(x1), _ptr(pk["shift"]), _ptr(pk["scale"])
        for i in range(_native.LPIPS_CONVS):
            a.conv_w[i], a.conv_wt[i], a.conv_b[i] = pk["conv_w"][i].data_ptr(), pk["conv_wt"][i].data_ptr(), pk["conv_b"][i].data_ptr()
        for k in range(_native.LPIPS_TAPS):
            a.lin[k] = pk["lin"][k].data_ptr()
        a.out, a.grad0, a.workspace, a.workspace_bytes = _ptr(out), _ptr(g0) if g0 is not None else None, _ptr(ws), bytes_
        return a

    st = _stream(x0)
    assert L.dgs_lpips_forward_backward(ctypes.byref(args(g0=None)), st) == INVALID          # NULL grad0
    assert L.dgs_lpips_forward_backward(ctypes.byref(args(H=15)), st) == INVALID
    assert L.dgs_lpips_forward_backward(ctypes.byref(args(W=15)), st) == INVALID
    assert L.dgs_lpips_forward_backward(ctypes.byref(args(bytes_=nbytes - 16)), st) == INVALID  # a workspace too small
    assert L.dgs_lpips_forward_backward(ctypes.byref(args()), st) == 0
    assert same_bytes(out.cpu(), want.reshape(-1).cpu())
    assert L.dgs_conv3x3_backward_data(ctypes.byref(_native.DgsConv3x3BackwardDataArgs()), None) == INVALID
    assert L.dgs_maxpool2x2_backward(ctypes.byref(_native.DgsMaxPool2x2BackwardArgs()), None) == INVALID
    assert L.dgs_lpips_tap_backward(ctypes.byref(_native.DgsLpipsTapBackwardArgs()), None) == INVALID
    assert L.dgs_lpips_pack_weights_transposed(ctypes.byref(_native.DgsLpipsPackArgs()), None) == INVALID
    assert L.dgs_lpips_grad_workspace_bytes(1, 15, 16) == 0 and L.dgs_lpips_grad_chunk(1, 16, 15) == 0


def check_workspace(L):
    """Bounded in N, and what the header states for 8 pairs of 256^2."""
    assert L.dgs_lpips_grad_chunk(16, 256, 256) == 8 and L.dgs_lpips_grad_chunk(3, 256, 256) == 3
    b = L.dgs_lpips_grad_workspace_bytes(8, 256, 256)
    assert b == L.dgs_lpips_grad_workspace_bytes(40, 256, 256) == L.dgs_lpips_grad_workspace_bytes(10 ** 6, 256, 256)
    per_image = 65536 * (3 + 270 + 128)
    assert 16 * per_image * 4 <= b <= 16 * per_image * 4 + (4 << 20)    # + one float per pixel and five per pair
    assert 0 < L.dgs_lpips_grad_workspace_bytes(1, 16, 16) < L.dgs_lpips_grad_workspace_bytes(2, 16, 16)
