"""The LPIPS-VGG forward (csrc/lpips.hip, include/dgs_lpips.h, dgs_amd.lpips) on the CPU-emulated build of the kernels: the checks of
tests/lpips_util.py (which states the bars), and the module's surface.  tests/test_lpips_gpu.py runs the same checks on the GPU.

Trimmed here, because an emulated run of them is no matter of seconds (the emulator switches fibers at every MFMA): the whole-network
cases (3, 32, 48) and (1, 24, 40) run on the GPU only; (2, 16, 16), (2, 35, 21) and (2, 17, 31) run here, 3 to 5 s each.  The
properties run on one 16 x 19 batch of three pairs, 'alone' for the middle pair only and 'chunked' with chunks of 2 only."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

import lpips_util as LU
from dgs_amd import _native
from dgs_amd import lpips as P

DEV = "cpu"
EMU_NET_CASES = [(2, 16, 16), (2, 35, 21), (2, 17, 31)]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", LU.CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_convolution_is_exact(case, relu):
    LU.check_conv_exact(DEV, *case, relu)


@pytest.mark.parametrize("case", LU.POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pool_is_exact(case):
    LU.check_pool_exact(DEV, *case)


@pytest.mark.parametrize("case", LU.TAP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_tap_kernel_against_fp64(case):
    LU.check_tap(DEV, *case)


@pytest.mark.parametrize("case", EMU_NET_CASES, ids=lambda c: "x".join(map(str, c)))
def test_network_against_fp64(case):
    LU.check_network(DEV, *case)


@pytest.mark.parametrize("which", LU.PROPERTIES)
def test_properties_bitwise(which):
    LU.check_property(DEV, which, thorough=False)


# ---- surface (no kernel runs unless stated) ----
def test_state_dict_names_round_trip_strictly():
    sd = LU.random_state_dict(3)
    m = P.LPIPS(net="vgg", lib=LU.lib_of(DEV))
    want = {f"net.{n}.{leaf}" for n in P.CONV_NAMES for leaf in ("weight", "bias")} | {f"lin{k}.model.1.weight" for k in range(5)} | {
        "scaling_layer.shift", "scaling_layer.scale"}
    assert set(m.state_dict()) == want
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert v.shape == sd[k].shape and torch.equal(v, sd[k]), k
    assert tuple(m.state_dict()["scaling_layer.shift"].shape) == (1, 3, 1, 1) and tuple(m.state_dict()["lin3.model.1.weight"].shape) == (1, 512, 1, 1)
    # the package registers the lin layers a second time, as lins.{k}: accepted and ignored
    dup = dict(sd)
    for k in range(5):
        dup[f"lins.{k}.model.1.weight"] = sd[f"lin{k}.model.1.weight"]
    P.LPIPS(net="vgg").load_state_dict(dup, strict=True)
    P.LPIPS(net="vgg", weights=dup)
    with pytest.raises(RuntimeError):
        P.LPIPS(net="vgg").load_state_dict({k: v for k, v in sd.items() if k != "net.slice3.12.bias"}, strict=True)
    assert not any(p.requires_grad for p in m.parameters()) and not m.training


def test_constructor_from_the_two_files():
    sd = LU.random_state_dict(4)
    index = {n: n.split(".")[1] for n in P.CONV_NAMES}
    vgg16 = {f"features.{i}.{leaf}": sd[f"net.{n}.{leaf}"] for n, i in index.items() for leaf in ("weight", "bias")}
    vgg16["classifier.0.weight"] = torch.zeros(2, 2)                       # torchvision's file holds the classifier too
    lin = {f"lin{k}.model.1.weight": sd[f"lin{k}.model.1.weight"] for k in range(5)}
    assert sorted(int(i) for i in index.values()) == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    with tempfile.TemporaryDirectory() as d:
        torch.save(vgg16, os.path.join(d, "vgg16.pth"))
        torch.save(lin, os.path.join(d, "vgg.pth"))
        a = P.LPIPS.from_files(os.path.join(d, "vgg16.pth"), os.path.join(d, "vgg.pth"))
    b = P.LPIPS.from_files(vgg16, lin)
    for m in (a, b):
        got = m.state_dict()
        assert set(got) == set(sd)
        for k in sd:
            assert torch.equal(got[k], sd[k]), k


def test_errors():
    L = LU.lib_of(DEV)
    with pytest.raises(ValueError):
        P.LPIPS(net="alex")
    with pytest.raises(ValueError):
        P.LPIPS(net="squeeze")
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no weights"):
        P.LPIPS(net="vgg", lib=L)(x, x)
    m = LU.model(DEV)
    with pytest.raises(NotImplementedError, match="input gradient"):
        m(x.clone().requires_grad_(True), x)
    with pytest.raises(NotImplementedError, match="input gradient"):
        m(x, x.clone().requires_grad_(True))
    with torch.no_grad():                                                  # as a metric it runs, and says nothing about a gradient
        assert not m(x.clone().requires_grad_(True), x).requires_grad
    with pytest.raises(ValueError, match="16 x 16"):
        m(torch.zeros(1, 3, 15, 16), torch.zeros(1, 3, 15, 16))
    with pytest.raises(ValueError, match="16 x 16"):
        m(torch.zeros(1, 3, 16, 15), torch.zeros(1, 3, 16, 15))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 16, 16), torch.zeros(2, 3, 16, 16))
    # the C ABI itself
    a = _native.DgsLpipsForwardArgs()
    a.N, a.H, a.W = 1, 15, 16
    assert L.dgs_lpips_forward(ctypes.byref(a), None) != 0 and L.dgs_lpips_workspace_bytes(1, 15, 16) == 0 and L.dgs_lpips_workspace_bytes(1, 16, 15) == 0
    assert L.dgs_conv3x3(ctypes.byref(_native.DgsConv3x3Args()), None) != 0
    assert L.dgs_maxpool2x2(ctypes.byref(_native.DgsMaxPool2x2Args()), None) != 0
    assert L.dgs_lpips_tap(ctypes.byref(_native.DgsLpipsTapArgs()), None) != 0
    assert L.dgs_lpips_pack_weights(ctypes.byref(_native.DgsLpipsPackArgs()), None) != 0
    assert L.dgs_conv3x3_packed_floats(0, 4) == 0 and L.dgs_conv3x3_packed_floats(3, 64) == 32 * 64 and L.dgs_conv3x3_packed_floats(64, 65) == 576 * 128


def test_workspace_is_bounded_in_n():
    L = LU.lib_of(DEV)
    assert L.dgs_lpips_chunk(16, 256, 256) == 8 and L.dgs_lpips_chunk(3, 256, 256) == 3 and L.dgs_lpips_chunk(5, 1024, 1024) == 1
    assert L.dgs_lpips_workspace_bytes(8, 256, 256) == L.dgs_lpips_workspace_bytes(40, 256, 256) == L.dgs_lpips_workspace_bytes(10 ** 6, 256, 256)
    assert 0 < L.dgs_lpips_workspace_bytes(1, 16, 16) < L.dgs_lpips_workspace_bytes(2, 16, 16)


def test_normalize_and_weight_refresh():
    """normalize=True maps (0, 1) to (-1, 1); an in-place change of a parameter reaches the packed copies (one small case, emulated)."""
    m = P.LPIPS(net="vgg", lib=LU.lib_of(DEV))
    m.load_state_dict(LU.random_state_dict(0), strict=True)
    x0, x1 = LU.images(1, 16, 16, seed=5)
    assert LU.same_bytes(m((x0 + 1) / 2, (x1 + 1) / 2, normalize=True), m(2 * ((x0 + 1) / 2) - 1, 2 * ((x1 + 1) / 2) - 1))
    packed = m.packed()
    assert m.packed() is packed                                            # nothing changed: nothing is rebuilt
    with torch.no_grad():
        m.lin_parameters()[0].mul_(2.0)
    assert m.packed() is not packed
    b = m.run(x0, x1, want_taps=True)["per_tap"]
    base = LU.model(DEV).run(x0, x1, want_taps=True)["per_tap"]
    assert LU.same_bytes(b[:, 0], 2 * base[:, 0]) and LU.same_bytes(b[:, 1:], base[:, 1:])


def test_struct_sizes_and_symbols():
    structs = ["DgsConv3x3Args", "DgsMaxPool2x2Args", "DgsLpipsPackArgs", "DgsLpipsTapArgs", "DgsLpipsForwardArgs"]
    src = '#include <stdio.h>\n#include "dgs_lpips.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({s}));' for s in structs) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        with open(c, "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(LU.ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    for s, n in zip(structs, sizes):
        assert ctypes.sizeof(getattr(_native, s)) == n, (s, ctypes.sizeof(getattr(_native, s)), n)
    import re
    header = open(os.path.join(LU.ROOT, "include", "dgs_lpips.h")).read()
    declared = set(re.findall(r"\b(dgs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_native.LPIPS_SYMBOLS)
    L = LU.lib_of(DEV)
    for name in _native.LPIPS_SYMBOLS:
        assert hasattr(L, name), name
