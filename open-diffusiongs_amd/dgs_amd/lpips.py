"""LPIPS-VGG on the device: what `lpips.LPIPS(net="vgg")` (version 0.1, lpips=True, spatial=False, eval mode) returns for two image
batches, computed by csrc/lpips.hip through include/dgs_lpips.h (which states the network and its arithmetic) -- in fp32, as
eval_scene_result.py of the reference runs it (no autocast), deterministically, with neither the `lpips` nor the `torchvision`
package behind it.  The default module is the metric (dgs_amd.metrics) and refuses an input that requires grad;
`LPIPS(..., differentiable=True)` is the trainer's perceptual term: its forward computes the gradient of every out[n] with respect to
the images in the same call (dgs_lpips_forward_backward) and stores it, so no activation outlives the call and memory is bounded by
the chunk, not by the batch.  The network is frozen: there is no weight gradient.

State dict.  Parameters and buffers carry the names of the `lpips` package, so `load_state_dict(lpips.LPIPS(net="vgg").state_dict())`
works strictly:
    net.slice1.{0,2}  net.slice2.{5,7}  net.slice3.{10,12,14}  net.slice4.{17,19,21}  net.slice5.{24,26,28}   .weight / .bias
    scaling_layer.shift, scaling_layer.scale    buffers [1, 3, 1, 1]
    lin{0..4}.model.1.weight                    [1, C, 1, 1], C = 64, 128, 256, 512, 512
    lins.{0..4}.model.1.weight                  the package's second registration of the same tensors: accepted and ignored
`LPIPS.from_files` takes the two files a user has: torchvision's vgg16 state dict (`features.{0,2,5,...,28}.{weight,bias}`) and the
package's `weights/v0.1/vgg.pth` (`lin{k}.model.1.weight`).
THESE NAMES ARE WRITTEN FROM MEMORY OF THE TWO PACKAGES.  Neither is installed where this library is built and tested, so they have not
been checked against them; the suite tests the arithmetic with seeded random weights against an fp64 restatement in torch.

No CPU fallback: a library without the LPIPS symbols is an error."""
import ctypes

import torch
import torch.nn as nn

from . import _native

CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
CONV_NAMES = ("slice1.0", "slice1.2", "slice2.5", "slice2.7", "slice3.10", "slice3.12", "slice3.14", "slice4.17", "slice4.19", "slice4.21",
              "slice5.24", "slice5.26", "slice5.28")
POOL_BEFORE = (2, 4, 7, 10)                  # a 2x2 maximum pool stands in front of these convolutions
TAP_AFTER = (1, 3, 6, 9, 12)                 # the taps: the ReLU output of these convolutions
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def _library(lib):
    L = lib or _native.lib()
    if not hasattr(L, "dgs_lpips_forward"):
        raise RuntimeError("dgs_amd: this library build predates the LPIPS network -- rebuild it (`python -m dgs_amd.build`)")
    return L


def _gradient_library(lib):
    L = _library(lib)
    if not hasattr(L, "dgs_lpips_forward_backward"):
        raise RuntimeError("dgs_amd: this library build predates the LPIPS input gradient -- rebuild it (`python -m dgs_amd.build`)")
    return L


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {rc}")


def pack_weights(weight, lib=None):
    """[Cout, Cin, 3, 3] -> the packed GEMM operand of dgs_conv3x3 (include/dgs_lpips.h 'packed weights'), on weight's device."""
    L = _library(lib)
    w = weight.detach().contiguous().float()
    cout, cin = int(w.shape[0]), int(w.shape[1])
    if tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"pack_weights: a [Cout, Cin, 3, 3] tensor expected, got {tuple(weight.shape)}")
    packed = torch.empty(int(L.dgs_conv3x3_packed_floats(cin, cout)), dtype=torch.float32, device=w.device)
    a = _native.DgsLpipsPackArgs(cin, cout, _ptr(w), _ptr(packed))
    _check(L.dgs_lpips_pack_weights(ctypes.byref(a), _stream(w)), "dgs_lpips_pack_weights")
    return packed


def pack_weights_transposed(weight, lib=None):
    """[Cout, Cin, 3, 3] -> the packed operand of dgs_conv3x3_backward_data: the convolution Cout -> Cin on the flipped, transposed
    weights, written straight from `weight`."""
    L = _gradient_library(lib)
    w = weight.detach().contiguous().float()
    cout, cin = int(w.shape[0]), int(w.shape[1])
    if tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"pack_weights_transposed: a [Cout, Cin, 3, 3] tensor expected, got {tuple(weight.shape)}")
    packed = torch.empty(int(L.dgs_conv3x3_packed_floats(cout, cin)), dtype=torch.float32, device=w.device)
    a = _native.DgsLpipsPackArgs(cin, cout, _ptr(w), _ptr(packed))
    _check(L.dgs_lpips_pack_weights_transposed(ctypes.byref(a), _stream(w)), "dgs_lpips_pack_weights_transposed")
    return packed


def conv3x3_backward_data(dy, packed_t, cin, mask=None, add=None, lib=None):
    """dy f32 [N, H, W, Cout] channels-last, packed_t = pack_weights_transposed(w) -> dx [N, H, W, cin] = (mask > 0 ? sum : 0) + add."""
    L = _gradient_library(lib)
    dy = dy.contiguous()
    n, h, w, cout = (int(d) for d in dy.shape)
    mask = mask.contiguous() if mask is not None else None
    add = add.contiguous() if add is not None else None
    assert all(t is None or tuple(t.shape) == (n, h, w, cin) for t in (mask, add))
    dx = torch.empty(n, h, w, cin, dtype=torch.float32, device=dy.device)
    a = _native.DgsConv3x3BackwardDataArgs(n, h, w, cin, cout, _ptr(dy), _ptr(packed_t), _ptr(mask), _ptr(add), _ptr(dx))
    _check(L.dgs_conv3x3_backward_data(ctypes.byref(a), _stream(dy)), "dgs_conv3x3_backward_data")
    return dx


def maxpool2x2_backward(x, dy, relu_mask=False, add=None, lib=None):
    """x f32 [N, H, W, C] (the pool's input), dy [N, H // 2, W // 2, C] -> dx [N, H, W, C]: dy routed to the first maximum of each
    window, then (x > 0 ? . : 0) with relu_mask, then + add."""
    L = _gradient_library(lib)
    x, dy = x.contiguous(), dy.contiguous()
    n, h, w, c = (int(d) for d in x.shape)
    assert tuple(dy.shape) == (n, h // 2, w // 2, c)
    add = add.contiguous() if add is not None else None
    assert add is None or add.shape == x.shape
    dx = torch.empty_like(x)
    a = _native.DgsMaxPool2x2BackwardArgs(n, h, w, c, _ptr(x), _ptr(dy), int(relu_mask), _ptr(add), _ptr(dx))
    _check(L.dgs_maxpool2x2_backward(ctypes.byref(a), _stream(x)), "dgs_maxpool2x2_backward")
    return dx


def tap_backward(f0, f1, lin, want_g1=True, lib=None):
    """The gradient of tap_distance(f0, f1, lin)[n] with respect to f0 (and f1) -> (g0, g1 or None), 0 where the feature itself is 0."""
    L = _gradient_library(lib)
    f0, f1, lin = f0.contiguous(), f1.contiguous(), lin.contiguous().reshape(-1)
    n, h, w, c = (int(d) for d in f0.shape)
    assert f1.shape == f0.shape and lin.numel() == c
    g0 = torch.empty_like(f0)
    g1 = torch.empty_like(f1) if want_g1 else None
    a = _native.DgsLpipsTapBackwardArgs(n, h, w, c, _ptr(f0), _ptr(f1), _ptr(lin), _ptr(g0), _ptr(g1))
    _check(L.dgs_lpips_tap_backward(ctypes.byref(a), _stream(f0)), "dgs_lpips_tap_backward")
    return g0, g1


def conv3x3(x, packed, bias, cout, relu=True, lib=None):
    """One layer on a channels-last activation: x f32 [N, H, W, Cin] -> [N, H, W, cout]."""
    L = _library(lib)
    x = x.contiguous()
    n, h, w, cin = (int(d) for d in x.shape)
    y = torch.empty(n, h, w, cout, dtype=torch.float32, device=x.device)
    a = _native.DgsConv3x3Args(n, h, w, cin, cout, _ptr(x), _ptr(packed), _ptr(bias), int(relu), _ptr(y))
    _check(L.dgs_conv3x3(ctypes.byref(a), _stream(x)), "dgs_conv3x3")
    return y


def maxpool2x2(x, lib=None):
    """x f32 [N, H, W, C] channels-last -> [N, H // 2, W // 2, C]."""
    L = _library(lib)
    x = x.contiguous()
    n, h, w, c = (int(d) for d in x.shape)
    y = torch.empty(n, h // 2, w // 2, c, dtype=torch.float32, device=x.device)
    a = _native.DgsMaxPool2x2Args(n, h, w, c, _ptr(x), _ptr(y))
    _check(L.dgs_maxpool2x2(ctypes.byref(a), _stream(x)), "dgs_maxpool2x2")
    return y


def tap_distance(f0, f1, lin, lib=None):
    """Two channels-last feature maps f32 [N, H, W, C] and lin [C] -> d [N] (include/dgs_lpips.h 'per tap')."""
    L = _library(lib)
    f0, f1, lin = f0.contiguous(), f1.contiguous(), lin.contiguous().reshape(-1)
    n, h, w, c = (int(d) for d in f0.shape)
    assert f1.shape == f0.shape and lin.numel() == c
    out = torch.empty(n, dtype=torch.float32, device=f0.device)
    ws = torch.empty(n * h * w, dtype=torch.float32, device=f0.device)
    a = _native.DgsLpipsTapArgs(n, h, w, c, _ptr(f0), _ptr(f1), _ptr(lin), _ptr(out), 1, _ptr(ws))
    _check(L.dgs_lpips_tap(ctypes.byref(a), _stream(f0)), "dgs_lpips_tap")
    return out


def tap_shapes(h, w):
    """[(h_k, w_k, C_k)] of the five taps for an input of h x w."""
    return [(h >> k, w >> k, c) for k, c in enumerate(TAP_CHANNELS)]


class _Holder(nn.Module):
    """A place in the module tree: it gives the parameters below it the package's names and computes nothing."""


class _Conv(nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin, k, k), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)


class _Lin(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(1, c, 1, 1), requires_grad=False)


class _LpipsFunction(torch.autograd.Function):
    """out [n] with the gradient of out[n] with respect to the inputs that require grad computed in the forward call and stored (the
    size of those inputs); backward multiplies the stored rows by grad_out[n].  Once differentiable: a second derivative raises."""

    @staticmethod
    def forward(ctx, module, in0, in1, chunk):
        need0, need1 = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        swap = need1 and not need0            # the library's first image set is the one that always gets a gradient
        r = module.run_with_gradient(in1 if swap else in0, in0 if swap else in1, both=need0 and need1, chunk=chunk)
        g0, g1 = (r["grad1"], r["grad0"]) if swap else (r["grad0"], r["grad1"])
        ctx.dtypes = (in0.dtype, in1.dtype)
        ctx.devices = (in0.device, in1.device)
        ctx.save_for_backward(*[g for g in (g0, g1) if g is not None])
        ctx.which = (g0 is not None, g1 is not None)
        return r["out"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)
        grads = []
        for i, have in enumerate(ctx.which):
            if not have:
                grads.append(None)
                continue
            g = saved.pop(0)
            grads.append((grad_out.to(g.device, g.dtype).reshape(-1, 1, 1, 1) * g).to(ctx.devices[i], ctx.dtypes[i]))
        return None, grads[0], grads[1], None


class LPIPS(nn.Module):
    """`LPIPS(net="vgg")`: forward(in0, in1, normalize=False) -> [n, 1, 1, 1] for in0, in1 f32 [n, 3, H, W] in (-1, 1) (in (0, 1)
    with normalize=True), H, W >= 16.  `weights`: a state dict with the package's names, or a path to one.  The module holds no
    weights of its own: until some are loaded, forward raises.

    differentiable=False (the default): the metric; an input that requires grad (with grad enabled) raises NotImplementedError.
    differentiable=True: such an input goes through one fused forward-and-backward call (dgs_lpips_forward_backward) that returns the
    same bytes as the metric and stores d out[n] / d input for the inputs that require grad (a target that does not costs no backward
    convolution); no activation outlives the call.  Under no_grad, or when no input requires grad, the metric's path runs."""

    def __init__(self, net="vgg", weights=None, lib=None, differentiable=False):
        super().__init__()
        if net != "vgg":
            raise ValueError(f"dgs_amd.lpips.LPIPS: only net='vgg' is built (asked for {net!r}); 'alex' and 'squeeze' are not")
        self._lib = lib
        self.differentiable = bool(differentiable)
        self.scaling_layer = _Holder()
        self.scaling_layer.register_buffer("shift", torch.tensor(SHIFT, dtype=torch.float32).reshape(1, 3, 1, 1))
        self.scaling_layer.register_buffer("scale", torch.tensor(SCALE, dtype=torch.float32).reshape(1, 3, 1, 1))
        self.net = _Holder()
        for name, (cin, cout) in zip(CONV_NAMES, CONV_CHANNELS):
            s, i = name.split(".")
            if not hasattr(self.net, s):
                self.net.add_module(s, _Holder())
            getattr(self.net, s).add_module(i, _Conv(cin, cout, 3))
        for k, c in enumerate(TAP_CHANNELS):
            lin = _Holder()
            lin.model = _Holder()
            lin.model.add_module("1", _Lin(c))
            self.add_module(f"lin{k}", lin)
        self._loaded = False
        self._packed, self._packed_version = None, None
        self.eval()
        if weights is not None:
            if not isinstance(weights, dict):
                weights = torch.load(weights, map_location="cpu")
            self.load_state_dict(weights, strict=True)

    @classmethod
    def from_files(cls, vgg16, lin, lib=None, differentiable=False):
        """vgg16: torchvision's `vgg16` state dict (or a path to it), of which `features.{0,2,...,28}.{weight,bias}` are read;
        lin: the package's `vgg.pth` (or a path), `lin{k}.model.1.weight`."""
        load = lambda x: x if isinstance(x, dict) else torch.load(x, map_location="cpu")
        vgg16, lin = load(vgg16), load(lin)
        sd = {}
        for name in CONV_NAMES:
            i = name.split(".")[1]
            for leaf in ("weight", "bias"):
                sd[f"net.{name}.{leaf}"] = vgg16[f"features.{i}.{leaf}"]
        for k in range(len(TAP_CHANNELS)):
            sd[f"lin{k}.model.1.weight"] = lin[f"lin{k}.model.1.weight"]
        m = cls(net="vgg", lib=lib, differentiable=differentiable)
        sd["scaling_layer.shift"], sd["scaling_layer.scale"] = m.scaling_layer.shift, m.scaling_layer.scale
        m.load_state_dict(sd, strict=True)
        return m

    def load_state_dict(self, state_dict, strict=True, **kw):
        state_dict = {k: v for k, v in state_dict.items() if not k.startswith("lins.")}     # the package's duplicate registration
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._loaded = True
        self._packed_version = None
        return out

    def conv_parameters(self):
        """[(weight, bias)] of the thirteen convolutions, in order."""
        out = []
        for name in CONV_NAMES:
            s, i = name.split(".")
            c = getattr(getattr(self.net, s), i)
            out.append((c.weight, c.bias))
        return out

    def lin_parameters(self):
        return [getattr(getattr(self, f"lin{k}").model, "1").weight for k in range(len(TAP_CHANNELS))]

    def packed(self, transposed=False):
        """The device-side operands (packed convolution weights, biases, lin vectors, shift and scale); rebuilt when a parameter's
        version, storage or device changes (load_state_dict, .to(), an in-place update).  transposed=True adds the operands of the data
        gradient (`conv_wt`) to the same cache the first time the gradient is asked for; they are invalidated with the rest."""
        tensors = list(self.parameters()) + list(self.buffers())
        version = tuple((p._version, p.data_ptr(), str(p.device), p.dtype) for p in tensors)
        if self._packed is None or version != self._packed_version:
            f = lambda t: t.detach().float().contiguous().reshape(-1)
            self._packed = dict(conv_w=[pack_weights(w, self._lib) for w, _ in self.conv_parameters()], conv_wt=None,
                                conv_b=[f(b) for _, b in self.conv_parameters()], lin=[f(w) for w in self.lin_parameters()],
                                shift=f(self.scaling_layer.shift), scale=f(self.scaling_layer.scale))
            self._packed_version = version
        if transposed and self._packed["conv_wt"] is None:
            self._packed["conv_wt"] = [pack_weights_transposed(w, self._lib) for w, _ in self.conv_parameters()]
        return self._packed

    def run(self, in0, in1, chunk=0, want_taps=False, want_features=False):
        """-> dict(out [n], per_tap [n, 5] or None, features: five [2, n, h_k, w_k, C_k] channels-last tensors or None)."""
        n, h, w = self._checked(in0, in1)
        L = _library(self._lib)
        dev = self.scaling_layer.shift.device
        x0, x1 = in0.detach().to(dev, torch.float32).contiguous(), in1.detach().to(dev, torch.float32).contiguous()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        if n == 0:
            return dict(out=out, per_tap=None, features=None)
        pk = self.packed()
        per_tap = torch.empty(n, _native.LPIPS_TAPS, dtype=torch.float32, device=dev) if want_taps else None
        feats = [torch.empty(2, n, hk, wk, c, dtype=torch.float32, device=dev) for hk, wk, c in tap_shapes(h, w)] if want_features else None
        nbytes = int(L.dgs_lpips_workspace_bytes(n, h, w))
        if nbytes == 0:
            raise ValueError(f"LPIPS: unsupported size n = {n}, {h} x {w}")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        a = _native.DgsLpipsForwardArgs()
        a.N, a.H, a.W, a.x0, a.x1, a.shift, a.scale = n, h, w, _ptr(x0), _ptr(x1), _ptr(pk["shift"]), _ptr(pk["scale"])
        for i in range(_native.LPIPS_CONVS):
            a.conv_w[i], a.conv_b[i] = pk["conv_w"][i].data_ptr(), pk["conv_b"][i].data_ptr()
        for k in range(_native.LPIPS_TAPS):
            a.lin[k] = pk["lin"][k].data_ptr()
        a.out, a.per_tap, a.chunk, a.workspace, a.workspace_bytes = _ptr(out), _ptr(per_tap), int(chunk), _ptr(ws), nbytes
        table = None
        if feats is not None:
            table = (ctypes.c_void_p * _native.LPIPS_TAPS)(*[f.data_ptr() for f in feats])
            a.features = ctypes.cast(table, ctypes.POINTER(ctypes.c_void_p))
        _check(L.dgs_lpips_forward(ctypes.byref(a), _stream(x0)), "dgs_lpips_forward")
        return dict(out=out, per_tap=per_tap, features=feats)

    def _checked(self, in0, in1):
        if not self._loaded:
            raise RuntimeError("dgs_amd.lpips.LPIPS: no weights have been loaded (load_state_dict, `weights=` or LPIPS.from_files); the "
                               "library ships none")
        if in0.shape != in1.shape or in0.dim() != 4 or in0.shape[1] != 3:
            raise ValueError(f"LPIPS: two [n, 3, H, W] tensors of one shape expected, got {tuple(in0.shape)} and {tuple(in1.shape)}")
        n, _, h, w = (int(d) for d in in0.shape)
        if h < 16 or w < 16:
            raise ValueError(f"LPIPS: images of {h} x {w} are smaller than 16 x 16, the last tap would be empty")
        return n, h, w

    def run_with_gradient(self, in0, in1, both=True, chunk=0, want_taps=False):
        """One dgs_lpips_forward_backward call -> dict(out [n], per_tap [n, 5] or None, grad0 [n, 3, H, W] = d out[n] / d in0[n],
        grad1 likewise or None when both is False).  Nothing here is recorded by autograd."""
        n, h, w = self._checked(in0, in1)
        L = _gradient_library(self._lib)
        dev = self.scaling_layer.shift.device
        x0, x1 = in0.detach().to(dev, torch.float32).contiguous(), in1.detach().to(dev, torch.float32).contiguous()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        grad0 = torch.empty(n, 3, h, w, dtype=torch.float32, device=dev)
        grad1 = torch.empty(n, 3, h, w, dtype=torch.float32, device=dev) if both else None
        per_tap = torch.empty(n, _native.LPIPS_TAPS, dtype=torch.float32, device=dev) if want_taps else None
        if n == 0:
            return dict(out=out, per_tap=per_tap, grad0=grad0, grad1=grad1)
        pk = self.packed(transposed=True)
        nbytes = int(L.dgs_lpips_grad_workspace_bytes(n, h, w))
        if nbytes == 0:
            raise ValueError(f"LPIPS: unsupported size n = {n}, {h} x {w}")
        if chunk:
            nbytes = int(L.dgs_lpips_grad_workspace_bytes(min(n, int(chunk)), h, w))
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        a = _native.DgsLpipsGradArgs()
        a.N, a.H, a.W, a.x0, a.x1, a.shift, a.scale = n, h, w, _ptr(x0), _ptr(x1), _ptr(pk["shift"]), _ptr(pk["scale"])
        for i in range(_native.LPIPS_CONVS):
            a.conv_w[i], a.conv_wt[i], a.conv_b[i] = pk["conv_w"][i].data_ptr(), pk["conv_wt"][i].data_ptr(), pk["conv_b"][i].data_ptr()
        for k in range(_native.LPIPS_TAPS):
            a.lin[k] = pk["lin"][k].data_ptr()
        a.out, a.per_tap, a.grad0, a.grad1 = _ptr(out), _ptr(per_tap), _ptr(grad0), _ptr(grad1)
        a.chunk, a.workspace, a.workspace_bytes = int(chunk), _ptr(ws), nbytes
        _check(L.dgs_lpips_forward_backward(ctypes.byref(a), _stream(x0)), "dgs_lpips_forward_backward")
        return dict(out=out, per_tap=per_tap, grad0=grad0, grad1=grad1)

    def forward(self, in0, in1, normalize=False):
        if torch.is_grad_enabled() and (in0.requires_grad or in1.requires_grad):
            if not self.differentiable:
                raise NotImplementedError("dgs_amd.lpips.LPIPS(differentiable=False) is the metric and computes no input gradient: call it "
                                          "under torch.no_grad(), or construct the module with differentiable=True to use it as a term of "
                                          "a loss")
            if normalize:
                in0, in1 = 2 * in0 - 1, 2 * in1 - 1
            self._checked(in0, in1)
            return _LpipsFunction.apply(self, in0, in1, 0).reshape(-1, 1, 1, 1)
        if normalize:
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        return self.run(in0, in1)["out"].reshape(-1, 1, 1, 1)
