"""Yardsticks and checks of the LPIPS tests (csrc/lpips.hip, include/dgs_lpips.h, dgs_amd.lpips).  Every check is a function of a
device: tests/test_lpips_emu.py runs it on the CPU-emulated build of the kernels, tests/test_lpips_gpu.py on the GPU.

The yardstick of the whole network is a restatement in torch of what `lpips.LPIPS(net="vgg")` computes (F.conv2d, F.max_pool2d and
the formulas of include/dgs_lpips.h), evaluated in fp64; the same code in fp32 on the CPU measures what a straightforward fp32
implementation loses.  The model has no weights where the suite runs: every test uses seeded random weights (convolutions
N(0, 2 / (9 Cin)), biases N(0, 0.05^2), lin weights uniform in [0, 0.1)).  Reads nothing outside the repository.

Bars.
  convolution, pool   exact: integer data whose partial sums stay below 2^24, compared with fp64 bit for bit, guard bands checked
  tap kernel          a sum of non-negative terms: relative error <= (C + H W + 16) 2^-24 against fp64
  tap features        relative L2 error against fp64 <= 8 x that of the fp32 restatement on the same case (measured with reference forms
                      only: a second blocked fp32 order lies at 0.98 - 2.63 x, a plain k-ordered fp32 chain, what the f32 MFMA
                      executes, at 1.59 - 3.28 x; 8 leaves 2.4 x over the worst)
  scalar              |d - d64| <= 8 |d32 - d64| + (512 + H W + 16) 2^-24 d64
"""
import ctypes
import functools
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "open-diffusiongs_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from dgs_amd import _native  # noqa: E402
from dgs_amd import lpips as P  # noqa: E402  (without the feature the module fails here)

U = 2.0 ** -24
FEATURE_FACTOR = 8.0
GUARD = 64
SENTINEL = 12345.0

CONV_CASES = [  # N, H, W, Cin, Cout
    (1, 1, 1, 64, 64),        # every tap but the centre is padding
    (2, 3, 5, 3, 64),         # the K = 27 path
    (1, 7, 9, 64, 128),
    (3, 5, 4, 128, 256),      # fewer pixels than one tile
    (2, 9, 15, 256, 512),     # tiles cross row and image boundaries
    (1, 16, 16, 512, 512),    # the full K
    (1, 6, 7, 32, 72),        # a Cout that is no multiple of the 64-wide wave tile
    (2, 5, 6, 5, 136),        # a Cin that is no multiple of the K chunk (two chunks on the scalar path), Cout 136 -> 192 padded
    (1, 19, 14, 64, 64),      # 266 pixels: a second, partly filled tile of 256
]
POOL_CASES = [(2, 2), (3, 5), (35, 21), (16, 16)]
TAP_CASES = [(2, 3, 5, 64), (3, 1, 1, 128), (1, 7, 9, 512), (2, 16, 16, 256), (1, 5, 53, 100)]   # N, H, W, C
NET_CASES = [(2, 16, 16), (3, 32, 48), (2, 35, 21), (1, 24, 40), (2, 17, 31)]                    # n, H, W


def lib_of(device):
    if str(device) == "cpu":
        from emu_util import emu_lib
        return emu_lib()
    return _native.lib()


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ---- weights ----
def random_state_dict(seed=0):
    """A state dict with the package's names, seeded."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (cin, cout) in zip(P.CONV_NAMES, P.CONV_CHANNELS):
        sd[f"net.{name}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[f"net.{name}.bias"] = torch.randn(cout, generator=g) * 0.05
    for k, c in enumerate(P.TAP_CHANNELS):
        sd[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g) * 0.1
    sd["scaling_layer.shift"] = torch.tensor(P.SHIFT).reshape(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(P.SCALE).reshape(1, 3, 1, 1)
    return sd


_models = {}


def model(device, seed=0):
    key = (str(device), seed)
    if key not in _models:
        m = P.LPIPS(net="vgg", lib=lib_of(device) if str(device) == "cpu" else None)
        m.load_state_dict(random_state_dict(seed), strict=True)
        _models[key] = m.to(device)
    return _models[key]


def images(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    x1 = (x0 + 0.3 * torch.randn(n, 3, h, w, generator=g)).clamp(-1, 1)
    return x0, x1


# ---- the restatement ----
def restatement(sd, in0, in1, dtype):
    """-> (out [n], per_tap [n, 5], features: five [2n, C, h, w] tensors), everything in `dtype` on the CPU."""
    return restatement_impl(sd, in0, in1, dtype, lambda t: t.detach().cpu().to(dtype))


def restatement_impl(sd, in0, in1, dtype, c):
    n = in0.shape[0]
    x = (torch.cat([c(in0), c(in1)]) - c(sd["scaling_layer.shift"])) / c(sd["scaling_layer.scale"])
    feats = []
    for i, name in enumerate(P.CONV_NAMES):
        if i in P.POOL_BEFORE:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, c(sd[f"net.{name}.weight"]), c(sd[f"net.{name}.bias"]), padding=1))
        if i in P.TAP_AFTER:
            feats.append(x)
    per_tap = []
    for k, f in enumerate(feats):
        fh = f / (f.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        d = (fh[:n] - fh[n:]) ** 2
        per_tap.append((d * c(sd[f"lin{k}.model.1.weight"])).sum(dim=1).mean(dim=(1, 2)))
    per_tap = torch.stack(per_tap, dim=1)
    return per_tap.sum(dim=1), per_tap, feats


def restatement_on(sd, in0, in1):
    """The fp32 restatement on the tensors' own device (the comparator of tools/lpips_bench.py) -> out [n]."""
    return restatement_impl(sd, in0, in1, torch.float32, lambda t: t.detach().to(in0.device, torch.float32))[0]


@functools.lru_cache(maxsize=None)
def net_reference(n, h, w):
    """The fp64 and fp32 restatements of a case, computed once and shared."""
    sd = random_state_dict(0)
    x0, x1 = images(n, h, w, seed=100 + n + h + w)
    return x0, x1, restatement(sd, x0, x1, torch.float64), restatement(sd, x0, x1, torch.float32)


def nchw(feature):
    """[2, n, h, w, C] channels-last -> [2n, C, h, w]."""
    return feature.flatten(0, 1).permute(0, 3, 1, 2).contiguous()


# ---- checks ----
def _guarded(numel, device):
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=device)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def check_conv_exact(device, N, H, W, Cin, Cout, relu):
    L = lib_of(device)
    g = torch.Generator().manual_seed(N * 1000 + H * 100 + W * 10 + Cin + Cout)
    x = torch.randint(-2, 3, (N, Cin, H, W), generator=g).float()
    w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=g).float()
    b = torch.randint(-3, 4, (Cout,), generator=g).float()
    want = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    assert float(want.abs().max()) < 2 ** 24
    if relu:
        want = F.relu(want)
    xd = x.permute(0, 2, 3, 1).contiguous().to(device)
    packed = P.pack_weights(w.to(device), L)
    assert packed.numel() == ((9 * Cin + 31) // 32 * 32) * ((Cout + 63) // 64 * 64)
    bd = b.to(device)
    buf, y = _guarded(N * H * W * Cout, device)
    a = _native.DgsConv3x3Args(N, H, W, Cin, Cout, _ptr(xd), _ptr(packed), _ptr(bd), int(relu), _ptr(y))
    assert L.dgs_conv3x3(ctypes.byref(a), _stream(xd)) == 0
    got = y.reshape(N, H, W, Cout).permute(0, 3, 1, 2).cpu()
    assert _guards_intact(buf.cpu()), "dgs_conv3x3 wrote outside its output"
    assert torch.equal(got.double(), want), f"max abs difference {float((got.double() - want).abs().max())}"
    assert torch.equal(P.conv3x3(xd, packed, bd, Cout, relu, L).cpu(), y.reshape(N, H, W, Cout).cpu())


def check_pool_exact(device, H, W):
    L = lib_of(device)
    N, C = 2, 7
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N, C, H, W, generator=g)
    want = F.max_pool2d(x, 2, 2) if H > 1 and W > 1 else x.new_zeros(N, C, H // 2, W // 2)
    xd = x.permute(0, 2, 3, 1).contiguous().to(device)
    buf, y = _guarded(want.numel(), device)
    a = _native.DgsMaxPool2x2Args(N, H, W, C, _ptr(xd), _ptr(y))
    assert L.dgs_maxpool2x2(ctypes.byref(a), _stream(xd)) == 0
    got = y.reshape(N, H // 2, W // 2, C).permute(0, 3, 1, 2).cpu()
    assert _guards_intact(buf.cpu()), "dgs_maxpool2x2 wrote outside its output"
    assert same_bytes(got, want)
    assert same_bytes(P.maxpool2x2(xd, L).cpu(), y.reshape(N, H // 2, W // 2, C).cpu())


def check_tap(device, N, H, W, C):
    """-> the measured relative error over its bar, per pair."""
    L = lib_of(device)
    g = torch.Generator().manual_seed(N + H * 7 + W * 13 + C)
    f0 = F.relu(torch.randn(N, H, W, C, generator=g) - 0.3)
    f1 = F.relu(f0 + 0.5 * torch.randn(N, H, W, C, generator=g))
    flat0, flat1 = f0.view(-1, C), f1.view(-1, C)
    flat0[0] = 0                                    # a pixel whose vector is all zero in f0 only,
    if flat0.shape[0] > 1:
        flat1[1] = 0                                # in f1 only,
    if flat0.shape[0] > 2:
        flat0[2] = 0                                # and in both: 0 / (0 + 1e-10) = 0
        flat1[2] = 0
    lin = torch.rand(C, generator=g) * 0.1
    h0 = f0.double() / (f0.double().pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    h1 = f1.double() / (f1.double().pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    want = ((h0 - h1) ** 2 * lin.double()).sum(-1).mean(dim=(1, 2))
    got = P.tap_distance(f0.to(device), f1.to(device), lin.to(device), L).cpu()
    again = P.tap_distance(f0.to(device), f1.to(device), lin.to(device), L).cpu()
    assert same_bytes(got, again)
    assert bool((P.tap_distance(f0.to(device), f0.to(device), lin.to(device), L).cpu() == 0).all())
    bar = (C + H * W + 16) * U
    zero = want == 0                                # both vectors zero at every pixel of the pair: exactly 0 is demanded
    assert bool((got[zero] == 0).all())
    ratio = torch.where(zero, torch.zeros_like(want), (got.double() - want).abs() / want.clamp_min(1e-300) / bar)
    print(f"tap N={N} H={H} W={W} C={C}: relative error / bar = {[round(float(r), 4) for r in ratio]} (bar {bar:.3e})")
    assert bool((ratio <= 1.0).all()), ratio
    return [float(r) for r in ratio]


def check_network(device, n, h, w):
    """-> rows (what, measured / bar) of the case: five tap features and the scalar of every pair."""
    x0, x1, (d64, t64, f64), (d32, t32, f32) = net_reference(n, h, w)
    m = model(device)
    r = m.run(x0.to(device), x1.to(device), want_taps=True, want_features=True)
    rows = []
    for k in range(5):
        got = nchw(r["features"][k]).cpu()
        assert got.shape == f64[k].shape, (got.shape, f64[k].shape)
        e, e32 = rel_l2(got, f64[k]), rel_l2(f32[k], f64[k])
        rows.append((f"tap{k} feature", e / (FEATURE_FACTOR * e32), e, e32))
    out, per_tap = r["out"].cpu().double(), r["per_tap"].cpu()
    assert same_bytes((((per_tap[:, 0] + per_tap[:, 1]) + per_tap[:, 2]) + per_tap[:, 3]) + per_tap[:, 4], r["out"].cpu())
    for i in range(n):
        bar = FEATURE_FACTOR * abs(float(d32[i]) - float(d64[i])) + (512 + h * w + 16) * U * float(d64[i])
        rows.append((f"pair{i} scalar", abs(float(out[i]) - float(d64[i])) / bar, float(out[i]), float(d64[i])))
    for what, ratio, a, b in rows:
        print(f"network n={n} {h}x{w} {what}: measured / bar = {ratio:.4f}   ({a:.6e} against {b:.6e})")
    assert all(ratio <= 1.0 for _, ratio, _, _ in rows), [(wh, ra) for wh, ra, _, _ in rows if ra > 1.0]
    fwd = m(x0.to(device), x1.to(device))
    assert tuple(fwd.shape) == (n, 1, 1, 1) and same_bytes(fwd.reshape(-1).cpu(), r["out"].cpu())
    return rows


PROPERTIES = ["identical", "repeat", "permute", "alone", "chunked"]
_base = {}


def _property_base(device, h=16, w=19):
    """Three pairs of 16 x 19 and their result with taps and features: computed once per device, shared and left unchanged."""
    if str(device) not in _base:
        x0, x1 = images(3, h, w, seed=7)
        x0, x1 = x0.to(device), x1.to(device)
        _base[str(device)] = (x0, x1, model(device).run(x0, x1, want_taps=True, want_features=True))
    return _base[str(device)]


def check_property(device, which, thorough=True):
    """One of PROPERTIES, bitwise.  thorough=False (the emulator): 'alone' takes the middle pair only, 'chunked' chunks of 2 only."""
    m = model(device)
    x0, x1, base = _property_base(device)
    out, taps = base["out"].cpu(), base["per_tap"].cpu()
    assert bool((out > 0).all())
    run = lambda a, b, **kw: m.run(a, b, want_taps=True, **kw)
    if which == "identical":          # lpips(x, x) is exactly 0, tap by tap
        same = run(x0, x0)
        assert bool((same["out"].cpu() == 0).all()) and bool((same["per_tap"].cpu() == 0).all())
    elif which == "repeat":           # two calls, equal bytes
        again = run(x0, x1)
        assert same_bytes(again["out"].cpu(), out) and same_bytes(again["per_tap"].cpu(), taps)
    elif which == "permute":          # permuting the batch permutes the outputs
        perm = torch.tensor([2, 0, 1])
        p = run(x0[perm.to(device)], x1[perm.to(device)])
        assert same_bytes(p["out"].cpu(), out[perm]) and same_bytes(p["per_tap"].cpu(), taps[perm])
    elif which == "alone":            # a pair alone gives what it gives inside the batch of 3
        for i in (range(3) if thorough else (1,)):
            one = run(x0[i:i + 1], x1[i:i + 1])
            assert same_bytes(one["out"].cpu(), out[i:i + 1]) and same_bytes(one["per_tap"].cpu(), taps[i:i + 1])
    elif which == "chunked":          # chunked calls equal the unchunked call, the features included
        for chunk in ((1, 2) if thorough else (2,)):
            c = m.run(x0, x1, chunk=chunk, want_taps=True, want_features=True)
            assert same_bytes(c["out"].cpu(), out) and same_bytes(c["per_tap"].cpu(), taps)
            for a, b in zip(c["features"], base["features"]):
                assert same_bytes(a.cpu(), b.cpu())
    else:
        raise ValueError(which)
