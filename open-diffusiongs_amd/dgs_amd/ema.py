"""Exponential moving average of the weights (include/dgs_ema.h, csrc/ema.hip, csrc/optim.hip).

The reference trains with `EMA(decay=0.9999)` + `EMAModelCheckpoint` unless `--use_ema` is off (launch.py:205-228): validation and test
run on the averaged weights (diffusionGS/utils/ema.py:167-181), every checkpoint is written twice, the second as `*-EMA.ckpt`
(utils/ema.py:202-215), and a resume picks the `-EMA` file up again (utils/ema.py:125-150).  As a callback on this engine that is three
torch ops per tensor and step, and per evaluation a device-to-host copy of all weights, a `load_state_dict` and a full refresh of the
engine's operand copies -- twice.  Here

    the shadows are kept by the launch that updates the parameters      FusedAdamW.attach_ema(ema): dgs_adamw_ema_step, + 8 B / parameter
    any other optimizer: one launch after its step                      ema.update(model): dgs_ema_apply
    evaluation on the averaged weights rewrites ONLY the engine's       with ema.swapped(model): dgs_ema_apply, once in and once out;
    bf16 / fp32 / transposed operand copies                             parameters, version counters, moments and gradients untouched
    the reference's checkpoint pair                                     ema.save_checkpoint(path, model, optimizer) / ema.load_checkpoint(path)

Arithmetic = the reference's non-apex `apply_ema` (utils/ema.py:94-101), bit for bit: diff = ema - w; diff.mul_(1 - decay); ema.sub_(diff).
The shadows of the parameters live in ONE flat fp32 buffer with the offsets of FusedAdamW's moments (optim.flat_offsets).
"""
import contextlib
import ctypes
import os
import warnings

import torch

from . import _native
from .dit import _stream
from .optim import flat_offsets

PREFIX = "shape_model."          # the Lightning system's name of the denoiser: the key prefix DGSDenoiser._load_pretrained strips


class EMA:
    def __init__(self, model, decay=0.9999, apply_ema_every_n_steps=1, start_step=0):
        """The reference callback's knobs (utils/ema.py:45-68; launch.py installs decay=0.9999).  The shadows start as a clone of the
        weights, as in its `on_train_start`."""
        if not (0 <= decay <= 1):
            raise ValueError("EMA decay value must be between 0 and 1")
        self.model = model
        self.lib = getattr(model, "_lib", None) or _native.lib()
        self.decay = float(decay)
        self.apply_ema_every_n_steps = int(apply_ema_every_n_steps)
        self.start_step = int(start_step)
        self.cur_step = None             # the step the EMA was last applied at (the reference's _cur_step)
        self.step = 0                    # applied optimizer updates seen by update(); with FusedAdamW the optimizer's own count leads
        self._undo = None
        named = list(model.named_parameters())
        sd = model.state_dict()
        self.param_names = [n for n, _ in named]
        if not set(self.param_names) <= set(sd):
            raise ValueError(f"EMA: parameters missing from the state dict: {sorted(set(self.param_names) - set(sd))[:4]}")
        self.keys = list(sd.keys())      # the reference zips state_dict().values() with its list: this order
        self.offsets, total = flat_offsets(p.numel() for _, p in named)
        self._shapes = {n: (off, p.numel(), tuple(p.shape)) for (n, p), off in zip(named, self.offsets)}
        self.flat = torch.zeros(total, dtype=torch.float32, device=named[0][1].device)
        # state-dict entries that are not parameters: floating-point ones are averaged like the rest (torch ops), others only carried
        self.extras = {k: v.detach().clone() for k, v in sd.items() if k not in self._shapes}
        self.restart_from(model)
        self._tables = {}

    @property
    def one_minus_decay(self):
        return 1.0 - self.decay          # a double: rounded once to fp32 where it is used, as torch's mul_(1.0 - decay) does

    def should_apply(self, step):
        """utils/ema.py:103-104.  `step` counts APPLIED optimizer updates."""
        return step != self.cur_step and step >= self.start_step and step % self.apply_ema_every_n_steps == 0

    # -- the shadows ------------------------------------------------------------------------------------------
    def shadow(self, key):
        if key in self._shapes:
            off, n, shape = self._shapes[key]
            return self.flat[off:off + n].view(shape)
        return self.extras[key]

    def shadow_state_dict(self):
        """{state-dict key: the shadow (a view, not a copy)} in the model's state-dict order: loads into a DGSDenoiser as it is."""
        return {k: self.shadow(k) for k in self.keys}

    def _bound(self, model):
        """The shadows, the tables and the swap all belong to the model this EMA was built for: the optional `model` argument of the
        public methods mirrors the reference callback's signatures and has to be that model."""
        if model is not None and model is not self.model:
            raise ValueError("EMA: built for another model (its shadows and launch tables belong to that one)")
        return self.model

    @torch.no_grad()
    def restart_from(self, model=None):
        """Shadows = the model's current weights."""
        self._check_not_swapped("restart_from")
        sd = self._bound(model).state_dict()
        self._same_keys(sd)
        for k in self.keys:
            self.shadow(k).copy_(sd[k])

    def _same_keys(self, sd):
        if set(sd) != set(self.keys):
            raise ValueError(f"EMA: state-dict keys differ from the model's this EMA was built for: {sorted(set(sd) ^ set(self.keys))[:4]}")

    def _averaged_extras(self):
        return [k for k, v in self.extras.items() if v.is_floating_point()]

    @torch.no_grad()
    def _torch_update(self, keys, gate=None):
        """The reference's loop over `keys`; gate (device float[1], the gradients' sum of squares): a non-finite one leaves the shadows
        as they are, like the launch it accompanies, without a host read."""
        if not keys:
            return
        sd = self.model.state_dict()
        keep = None if gate is None else torch.isfinite(gate.reshape(-1)[:1])
        for k in keys:
            e = self.shadow(k)
            d = e - sd[k]
            d.mul_(1.0 - self.decay)
            if keep is not None:
                d = torch.where(keep, d, torch.zeros((), dtype=d.dtype, device=d.device))      # e - 0 is e
            e.sub_(d)

    # -- called by FusedAdamW ------------------------------------------------------------------------------------
    def _applied_by_optimizer(self, step, covered, grad_sumsq):
        self._undo, self.cur_step, self.step = (self.cur_step, self.step), step, step
        cov = set(covered)
        self._torch_update([n for n in self.param_names if n not in cov] + self._averaged_extras(), grad_sumsq)

    def _step_was_skipped(self, step):
        if self.cur_step == step and self._undo is not None:
            (self.cur_step, self.step), self._undo = self._undo, None

    # -- tables of the standalone launch -------------------------------------------------------------------------
    def _table(self, kind, model):
        """kind 'update': every parameter, no copies.  kind 'swap': every state-dict entry the engine keeps an operand copy of
        (DitEngine.weight_destinations: the training path's transposed copies included once they exist)."""
        sd = model.state_dict()
        if kind == "update":
            items = [(n, sd[n], None, None) for n in self.param_names]
            key = tuple(sd[n].data_ptr() for n in self.param_names)
        else:
            eng = model.engine()
            dst = eng.weight_destinations()
            if not set(dst) <= set(self.keys):
                raise RuntimeError(f"EMA: the engine keeps copies of entries this EMA has no shadow of: {sorted(set(dst) - set(self.keys))[:4]}")
            items = [(n, sd[n], c, ct) for n, (c, ct) in dst.items()]
            key = (id(eng), id(eng._train)) + tuple(sd[n].data_ptr() for n in dst)
        hit = self._tables.get(kind)
        if hit is not None and hit[3] == key:
            return hit
        entries = []
        for name, p, copy, copy_t in items:
            s = self.shadow(name)
            if p.dtype != torch.float32 or not p.is_contiguous() or s.dtype != torch.float32 or p.device != s.device:
                raise RuntimeError(f"EMA: {name}: fp32 contiguous weights on the shadows' device only")
            e = _native.DgsEmaTensor()
            e.p, e.ema = p.data_ptr(), s.data_ptr()
            rows, cols = (int(p.shape[0]), p.numel() // int(p.shape[0])) if p.dim() >= 2 else (1, p.numel())
            e.rows, e.cols = rows, cols
            if copy is not None:
                if copy.numel() != p.numel() or not copy.is_contiguous():
                    raise RuntimeError(f"EMA: engine copy of {name} has another layout")
                e.copy = copy.data_ptr()
                e.copy_kind = _native.OPTIM_COPY_BF16 if copy.dtype == torch.bfloat16 else _native.OPTIM_COPY_F32
            if copy_t is not None:
                if tuple(copy_t.shape) != (cols, rows) or copy_t.dtype != torch.bfloat16 or not copy_t.is_contiguous():
                    raise RuntimeError(f"EMA: transposed engine copy of {name} has another layout")
                e.copy_t = copy_t.data_ptr()
            entries.append(e)
        host = (_native.DgsEmaTensor * len(entries))(*entries)
        n_tiles = int(self.lib.dgs_ema_plan(host, len(entries)))
        if n_tiles <= 0:
            raise RuntimeError("EMA: dgs_ema_plan rejected the tensor table")
        raw = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(self.flat.device)
        self._tables[kind] = (raw, len(entries), n_tiles, key)
        return self._tables[kind]

    def _launch(self, table, update, source):
        raw, n, n_tiles, _ = table
        a = _native.DgsEmaArgs()
        a.tensors, a.n_tensors, a.n_tiles = raw.data_ptr(), n, n_tiles
        a.one_minus_decay, a.update, a.copy_source = self.one_minus_decay, int(update), int(source)
        rc = self.lib.dgs_ema_apply(ctypes.byref(a), _stream(self.flat.device))
        if rc != 0:
            raise RuntimeError(f"dgs_ema_apply: {_native.status_string(self.lib, rc)} (status {rc})")

    # -- the update after a step of any other optimizer --------------------------------------------------------------
    def _check_not_swapped(self, what):
        if getattr(self.model, "_ema_swapped", False):
            raise RuntimeError(f"EMA: {what} inside `ema.swapped(model)`: the engine's copies hold the averaged weights")

    @torch.no_grad()
    def update(self, model=None, step=None):
        """Call right after an optimizer step that was actually taken (FusedAdamW with attach_ema does this itself, inside its launch).
        step: the count of applied updates (default: one more than at the last call).  One launch over all parameters; returns
        whether the schedule selected this step."""
        model = self._bound(model)
        self._check_not_swapped("ema.update")
        step = self.step + 1 if step is None else int(step)
        self.step = step
        if not self.should_apply(step):
            return False
        self.cur_step = step
        self._launch(self._table("update", model), 1, _native.EMA_SOURCE_NONE)
        self._torch_update(self._averaged_extras())
        return True

    # -- evaluation on the averaged weights ----------------------------------------------------------------------------
    @contextlib.contextmanager
    def swapped(self, model=None):
        """Inside the block the engine computes with the averaged weights: its bf16 / fp32 / transposed operand copies are written
        from the shadows (one launch, on the current stream) and from the parameters again on the way out.  The parameters, their
        version counters, the optimizer's moments and the flat gradient buffer are untouched, so `model.engine()` sees nothing to
        refresh and captured graphs replay on the same buffers.  Optimizer steps, `update`, a second entry and anything that would
        rewrite the shadows or make the engine refresh its copies from the raw weights (`model.load_state_dict` followed by
        `model.engine()`, `refresh_engine_weights`) raise while swapped."""
        model = self._bound(model)
        self._check_not_swapped("entering `swapped` again")
        model.engine()                       # built, and following the parameters
        with torch.no_grad():
            self._launch(self._table("swap", model), 0, _native.EMA_SOURCE_EMA)
        model._ema_swapped = True
        try:
            yield self
        finally:
            model._ema_swapped = False               # first: engine() may refresh again (it refused to inside the block)
            with torch.no_grad():
                self._launch(self._table("swap", model), 0, _native.EMA_SOURCE_P)     # planned again if copies were added meanwhile

    # -- state -----------------------------------------------------------------------------------------------
    def state_dict(self, with_weights=True):
        d = dict(cur_step=self.cur_step, step=self.step, decay=self.decay, apply_ema_every_n_steps=self.apply_ema_every_n_steps,
                 start_step=self.start_step)
        if with_weights:
            d["shadows"] = {k: v.detach().clone() for k, v in self.shadow_state_dict().items()}
        return d

    @torch.no_grad()
    def load_state_dict(self, sd):
        if "shadows" in sd:
            self._check_not_swapped("loading shadows")
        self.cur_step = None if sd.get("cur_step") is None else int(sd["cur_step"])
        self.step = int(sd.get("step", self.cur_step or 0))
        self.decay = float(sd.get("decay", self.decay))
        self.apply_ema_every_n_steps = int(sd.get("apply_ema_every_n_steps", self.apply_ema_every_n_steps))
        self.start_step = int(sd.get("start_step", self.start_step))
        self._undo = None
        if "shadows" in sd:
            self._load_shadows(sd["shadows"])

    def _load_shadows(self, weights):
        self._check_not_swapped("loading shadows")
        self._same_keys(weights)
        for k in self.keys:
            self.shadow(k).copy_(weights[k])

    # -- data parallel: every rank starts from the source rank's shadows, as it starts from its parameters -------------------------
    @torch.no_grad()
    def broadcast_shadows(self, src=0, group=None):
        """The init-time companion of parallel.broadcast_parameters: the shadows were cloned (or loaded) before the ranks' parameters
        were made equal, so they follow the same source rank -- freshly cloned or resumed from a checkpoint alike -- together with the
        schedule's state.  Once, at construction of the trainer; no collective per step.  Returns the bytes sent."""
        import torch.distributed as dist
        if not dist.is_initialized() or dist.get_world_size(group) == 1:
            return 0
        self._check_not_swapped("broadcast_shadows")
        sent = 0
        for t in [self.flat] + list(self.extras.values()):
            dist.broadcast(t, src=src, group=group)
            sent += t.numel() * t.element_size()
        state = torch.tensor([-1 if self.cur_step is None else self.cur_step, self.step], dtype=torch.int64, device=self.flat.device)
        dist.broadcast(state, src=src, group=group)
        cur, self.step = int(state[0]), int(state[1])
        self.cur_step, self._undo = (None if cur < 0 else cur), None
        return sent

    # -- the reference's checkpoint pair ----------------------------------------------------------------------------
    @staticmethod
    def ema_path(path):
        if not path.endswith(".ckpt"):
            raise ValueError("EMA checkpoints are named *.ckpt / *-EMA.ckpt")
        if path.endswith("-EMA.ckpt"):
            raise ValueError("this IS an -EMA.ckpt path: give the plain checkpoint's")
        return path[:-len(".ckpt")] + "-EMA.ckpt"          # the file's own extension only, not a directory named x.ckpt

    def save_checkpoint(self, path, model=None, optimizer=None):
        """Two files in the Lightning layout DGSDenoiser._load_pretrained reads: `path` with the raw weights, and its `-EMA.ckpt`
        sibling with the shadows in their place (EMAModelCheckpoint._save_checkpoint, utils/ema.py:202-215).  Returns both paths."""
        model = self._bound(model)
        second = self.ema_path(path)
        sd = model.state_dict()
        self._same_keys(sd)
        rest = {"ema": self.state_dict(with_weights=False)}
        if optimizer is not None:
            rest["optimizer_states"] = [optimizer.state_dict()]
        torch.save(dict(rest, state_dict={PREFIX + k: sd[k].detach().cpu() for k in self.keys}), path)
        torch.save(dict(rest, state_dict={PREFIX + k: v.detach().cpu() for k, v in self.shadow_state_dict().items()}), second)
        return path, second

    @torch.no_grad()
    def load_checkpoint(self, path, optimizer=None):
        """Resume (EMA.on_load_checkpoint, utils/ema.py:125-150): the file's weights go into the model (and its optimizer state into
        `optimizer`, when both are given); a path ending in `-EMA.ckpt` means the loaded weights ARE the main weights and the shadows
        restart from them; otherwise the shadows come from the sibling `-EMA.ckpt`, or -- with a warning -- restart when there is none."""
        self._check_not_swapped("load_checkpoint")
        ck = torch.load(path, map_location="cpu")
        self.model._load_pretrained({"state_dict": ck["state_dict"]})
        if optimizer is not None and ck.get("optimizer_states"):
            optimizer.load_state_dict(ck["optimizer_states"][0])
        if "ema" in ck:
            self.load_state_dict(ck["ema"])
        if path.endswith("-EMA.ckpt"):
            self.restart_from(self.model)
        elif os.path.exists(self.ema_path(path)):
            other = torch.load(self.ema_path(path), map_location="cpu")["state_dict"]
            self._load_shadows({k[len(PREFIX):]: v for k, v in other.items() if k.startswith(PREFIX)})
        else:
            warnings.warn("we were unable to find the associated EMA weights when re-loading, training will start with new EMA weights.",
                          UserWarning)
            self.restart_from(self.model)
        return ck
