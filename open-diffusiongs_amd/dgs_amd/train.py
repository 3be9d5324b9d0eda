"""One data-parallel training step of the hot path (what PointDiffusionSystem.training_step does around the model,
systems/diffusion_gs_system.py:71-128, minus the parts that are out of scope: the LPIPS network's weights -- the slot takes dgs_amd.lpips.LPIPS(differentiable=True) with
weights of the user's, or any network -- Lightning, logging back ends and data loading).

`train_step(clean batch)` after `configure_objective(diffusion, loss, perceptual)` is the reference's step: the noise and timestep
draws, q_sample and the xyz target (ONE launch, dgs_train_inputs), every loss term the library has on the device -- MSE, SSIM,
points-distribution, xyz, the perceptual slot -- under the `[start_step, start_value, end_value, end_step]` weight schedules of the
shipped configs.  `step(batch, t, target)` is the same loop on views somebody else noised, with the MSE (+ SSIM) term:

    gaussians = model.image_to_gaussians(noisy views)          DiT forward, activations saved / per-block recompute   (HIP)
    renders   = model.render_gaussians(gaussians, cameras)     all b*v views, one launch sequence                     (HIP)
    loss      = mean((renders - target)^2)                     the reference's lambda_mse term                        (HIP: dgs_amd.losses)
                [+ lambda_ssim * mean(1 - ssim(renders, target))   with DataParallelTrainer(lambda_ssim=...): one fused loss node]
    loss.backward()                                            rasterizer backward + DiT backward                     (HIP)
      `- per finished gradient group: all-reduce of the buckets it completes, on RCCL's stream, WHILE the backward of the
         earlier blocks is still being enqueued / executed                                                           (dgs_amd.parallel)
    optimizer step on the fp32 master parameters               torch.optim (AdamW in the reference configs)
    refresh of the engine's bf16 / transposed weight copies    in place

Lightning DDP in the reference (`strategy: ddp_find_unused_parameters_true`, configs/diffusionGS_rel.yaml:80;
scripts/train_obj_stage1.sh:5-7) reduces ~74 buckets of 25 MB behind autograd hooks.  Here dgs_dit_backward writes every
gradient into ONE flat fp32 buffer in backward-completion order and calls back after each block (DgsDitBackwardArgs.block_done);
the callback launches every bucket that just became final.  The parameters' .grad tensors ARE views of that buffer: the
collective reduces them in place and nothing is copied in or out.  Averaging is folded into the loss scale.
"""
import contextlib

import torch

from . import losses
from .parallel import BucketedAllReduce, GradNorm, broadcast_parameters


class DataParallelTrainer:
    """Owns the model's training hooks while it lives: `.grad` of every parameter is a view of the engine's flat gradient buffer,
    the backward writes there in place and reports finished groups to the bucketed all-reduce.  `close()` (or leaving the `with`
    block) hands the model back: a later plain `loss.backward()` then returns gradients through autograd again."""

    def __init__(self, model, optimizer, bucket_bytes=None, accumulate_grad_batches=1, group=None, compress=None, force_collectives=False,
                 max_grad_norm=None, broadcast_from=0, deterministic=None, lambda_ssim=None, ema=None):
        """deterministic (default on; DGS_RASTER_DETERMINISTIC=0 or False turns it off): the rasterizer backward without floating-point
        atomics (dgs_raster.h `scratch`), which makes the WHOLE step bit-reproducible -- the DiT backward, the bucketed all-reduce
        order, the norm and the AdamW launch already are -- for +0.10 of 1.07 ms of rasterizer backward at 4 views of 256^2
        (profiles/r04_raster_deterministic_ab.txt), ~0.1 % of the step, in trained-like scenes, and +1.6 % of the step (90.9 -> 92.4 ms,
        profiles/r05_train_det_alloc.txt) in the densest case the bench has: 4 x 10 views of random-init Gaussians, 634 M instances,
        45 GB of scratch (36 bytes per instance slot; past `backend.deterministic_budget` = 64 GiB the atomic form runs and
        `backend.last_backward_deterministic` says so).  Two runs from the same state then hold identical parameters,
        and so do the ranks of a data-parallel job after every step (tests/test_optim.py, tests/test_parallel_gloo.py).
        max_grad_norm: global-norm gradient clip (Lightning `gradient_clip_val`; the reference trains with 0.5,
        configs/diffusionGS_rel.yaml:76-77) -- the norm's partial sums are taken bucket by bucket behind each bucket's all-reduce and
        the scale is applied inside the optimizer launch (FusedAdamW) or as one in-place scale of the flat buffer (any other optimizer).
        broadcast_from: the rank whose parameters every rank starts from (DDP's init-time broadcast); None skips it.
        lambda_ssim: None (default) trains on the MSE term through losses.mse_psnr, as before.  A float -- 0.0 included: the reference
        evaluates and logs the term at weight 0 -- routes the step through losses.image_losses (loss = l2.mean() + lambda_ssim *
        ssim_loss.mean(), one fused backward launch) and keeps the per-sample term in `last_ssim_loss`.
        ema: a dgs_amd.ema.EMA of this model (the reference's EMA callback, launch.py:205-228).  FusedAdamW keeps the shadows inside its
        update launch; after any other optimizer's step -- when it was taken -- `ema.update(model)` is one more launch.  The EMA was
        built before this trainer, i.e. before `broadcast_from` made the ranks' parameters equal: its shadows (cloned or loaded from
        a checkpoint) are broadcast from the same rank here, once; after that no collective is needed, equal parameters and equal
        shadows stay equal.  `with trainer.evaluate():` runs on the averaged weights."""
        self.model, self.opt = model, optimizer
        import os
        if deterministic is None:
            deterministic = os.environ.get("DGS_RASTER_DETERMINISTIC", "1") not in ("", "0")
        self.deterministic = bool(deterministic)
        renderer = getattr(model, "gs_renderer", None)
        self._renderer, self._private_backend = renderer, False
        self._raster_backend = renderer.backend() if renderer is not None and hasattr(renderer, "backend") else None
        if renderer is not None and getattr(renderer, "_backend", "absent") is None and self._raster_backend is not None:
            # the model renders through the process-wide default backend: the trainer's choice (deterministic backward) must not leak to
            # its other users, so the model gets a backend of its own for as long as the trainer lives (same library, same exponential;
            # its plans learn their shapes again on the first step)
            from .raster import RasterBackend
            own = RasterBackend(lib=self._raster_backend.lib, exact_exp=self._raster_backend.exact_exp)
            own.deterministic_budget = self._raster_backend.deterministic_budget
            renderer._backend, self._raster_backend, self._private_backend = own, own, True
        self._raster_was_deterministic = getattr(self._raster_backend, "deterministic", None)
        self._raster_was_budget = getattr(self._raster_backend, "deterministic_budget", None)
        if self._raster_backend is not None:
            self._raster_backend.deterministic = self.deterministic
        self.accumulate = int(accumulate_grad_batches)
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm else None
        self.broadcast_bytes = 0
        if broadcast_from is not None:
            self.broadcast_bytes = broadcast_parameters(model, src=broadcast_from, group=group)
            if self.broadcast_bytes:
                model.refresh_engine_weights()
        eng = model.engine()
        self.fg = eng._train_state()["fg"]
        if next(model.parameters()).device != self.fg.flat.device:
            raise RuntimeError("DataParallelTrainer: the module's parameters must live on the engine's device (model.to(device))")
        self.norm = GradNorm(self.fg.flat, getattr(model, "_lib", None) or eng.lib) if self.max_grad_norm else None
        self.last_grad_sumsq = None      # device float[1] of the last step (its square root is the norm BEFORE clipping, as clip_grad_norm_ returns)
        self.reducer = BucketedAllReduce(self.fg.flat, bucket_bytes, group=group, compress=compress, force_collectives=force_collectives,
                                         norm=self.norm)
        self.world = self.reducer.world
        self._accum = torch.zeros_like(self.fg.flat) if self.accumulate > 1 else None      # allocated lazily too when a batch needs splitting
        self._summed_to = 0
        self._use_accum = False
        self._last_micro = True
        self._layers = eng.layers
        model._grads_in_place = True
        model._block_hook = self._on_gradients_final
        self._attach_grads()
        self.ema = ema
        if ema is not None and ema.model is not model:
            raise ValueError("DataParallelTrainer: the EMA was built for another model")
        if ema is not None and self.broadcast_bytes:
            self.broadcast_bytes += ema.broadcast_shadows(src=broadcast_from, group=group)
        if ema is not None and getattr(optimizer, "refreshes_engine", False):
            optimizer.attach_ema(ema)
        self.lambda_ssim = None if lambda_ssim is None else float(lambda_ssim)
        self.last_psnr = None
        self.last_ssim_loss = None       # [b] of the last micro-batch when lambda_ssim is set
        self.lead_probe = None           # a list: every block_done callback appends (stage, host time, event recorded on the compute stream)
        self._objective = None           # configure_objective: (diffusion, {lambda_*: number | schedule}, perceptual)
        self.global_step = 0             # calls of train_step (a plain int: set it when resuming); the schedules read it
        self.epoch = 0                   # read by schedules whose end_step is a float (utils/misc.py:89-93); the caller advances it
        self.last_terms = None           # train_step: {"loss_*": detached mean, "lambda_*": the weight used, "timesteps", "x_t", "loss"}

    def close(self):
        """Give the model back: no in-place gradients, no per-block hook; the parameters keep COPIES of their last gradients."""
        m = self.model
        if getattr(m, "_block_hook", None) == self._on_gradients_final:
            m._block_hook = None
            m._grads_in_place = False
            for p in m.parameters():
                if p.grad is not None:
                    p.grad = p.grad.clone()
            if self._private_backend:
                self._renderer._backend = None                 # back to the process-wide default backend, which was never touched
            elif self._raster_backend is not None and self._raster_was_deterministic is not None:
                self._raster_backend.deterministic = self._raster_was_deterministic
                self._raster_backend.deterministic_budget = self._raster_was_budget

    def evaluate(self):
        """Context manager: inside it the engine computes with the EMA weights (`ema.swapped(model)`: only its operand copies are
        rewritten, and written back on the way out).  Without an EMA: nothing happens."""
        return self.ema.swapped(self.model) if self.ema is not None else contextlib.nullcontext()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _attach_grads(self):
        """.grad of every parameter = its slice of the flat buffer (adaLN slices included): written by the backward, reduced
        in place by the collectives, read by the optimizer."""
        views = self.model.engine().grad_views()
        for n, p in self.model.named_parameters():
            v = views[n].reshape(p.shape)
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                p.grad = v

    def _end_of_stage(self, stage):
        if stage < 0:
            return self.fg.flat.numel()
        if stage >= self._layers:
            return self.fg.end_of("head_ada_b")
        return self.fg.end_of(f"{stage}.ada_b")

    def _on_gradients_final(self, stage):
        """Host callback from inside dgs_dit_backward: flat[:end] is final once the kernels enqueued so far have run."""
        if not self._last_micro:
            return
        if self.lead_probe is not None:                          # measurement (bench.py): how far the host runs ahead of the device here
            import time
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.lead_probe.append((stage, time.perf_counter(), ev))
        end = self._end_of_stage(stage)
        if self._use_accum and end > self._summed_to:             # fold in the earlier micro-batches, slice by slice
            self.fg.flat[self._summed_to:end] += self._accum[self._summed_to:end]
            self._summed_to = end
        self.reducer.ready_up_to(end, tag=stage)

    def _check_open(self):
        m = self.model
        if m._block_hook != self._on_gradients_final:
            raise RuntimeError("DataParallelTrainer.step after close() (or another trainer took the model over)")
        if getattr(m, "_ema_swapped", False):
            raise RuntimeError("DataParallelTrainer.step inside `evaluate()` / `ema.swapped(model)`: the engine holds the averaged weights")

    def step(self, batch, t, target, render_c2w=None, render_fxfycxcy=None):
        """batch: dict(image, ray_o, ray_d, c2w, fxfycxcy) like the reference's input_batch (leading dim = accumulate *
        per-micro-batch size when accumulate_grad_batches > 1); target [b, v, 3, H, W].  Returns the (local) mean loss."""
        m = self.model
        self._check_open()
        c2w = batch["c2w"] if render_c2w is None else render_c2w
        k = batch["fxfycxcy"] if render_fxfycxcy is None else render_fxfycxcy

        def micro_loss(sl, rendered, _aligned, _K):
            if self.lambda_ssim is None:
                loss, _l2, self.last_psnr = losses.mse_psnr(rendered, target[sl].to(rendered.dtype), lib=getattr(m, "_lib", None))
            else:
                loss, _l2, self.last_psnr, ssim_term = losses.image_losses(rendered, target[sl].to(rendered.dtype), 1.0, self.lambda_ssim,
                                                                            lib=getattr(m, "_lib", None))
                self.last_ssim_loss = ssim_term.detach()
            return loss

        return self._optimizer_step(batch["image"], batch["ray_o"], batch["ray_d"], t, c2w, k, micro_loss)

    def _optimizer_step(self, image, ray_o, ray_d, t, c2w, k, micro_loss):
        """One optimizer step over the local batch, shared by `step` and `train_step`: micro-batches and accumulation, per micro-batch
        the forward, the render, `micro_loss(slice, rendered, aligned, micro-batches) -> scalar` and its backward; then the all-reduce,
        the clip, the update, the EMA and the refresh.  Returns the mean of the micro-batches' losses."""
        m, K = self.model, self.accumulate
        self._attach_grads()
        H, W = image.shape[3], image.shape[4]
        nb = image.shape[0]
        assert nb % K == 0, "batch size must be a multiple of accumulate_grad_batches"
        mb = nb // K
        limit = getattr(m, "MAX_DIFFERENTIABLE_BATCH", 4)
        if mb > limit:
            # one dgs_dit_forward_train / dgs_dit_backward call takes <= 4 samples: a larger per-rank batch (the reference's scene
            # configurations: 12 at 512^2, 24 at 256^2; configs/diffusionGS_scene_512.yaml:16) runs as micro-batches inside THIS
            # optimizer step -- same gradient (mean over the whole batch), one all-reduce, one clip, one update
            c = -(-mb // limit)
            while mb % c:
                c += 1
            K, mb = K * c, mb // c
            if self._accum is None:
                self._accum = torch.zeros_like(self.fg.flat)
        total = 0.0
        self._summed_to = 0
        self._use_accum = K > 1
        self._micro_batches = K
        for j in range(K):
            sl = slice(j * mb, (j + 1) * mb)
            self._last_micro = j == K - 1
            params, aligned = m.image_to_gaussians(image[sl], ray_o[sl], ray_d[sl], t[sl])
            rendered = m.render_gaussians(params, c2w[sl], k[sl], H, W)
            loss = micro_loss(sl, rendered, aligned, K)
            (loss * (1.0 / (K * self.world))).backward()       # mean over micro-batches and ranks folded into the scale
            total = total + loss.detach()
            if not self._last_micro:
                if j == 0:
                    self._accum.copy_(self.fg.flat)
                else:
                    self._accum += self.fg.flat
        self.reducer.finish(average=False)
        ema_after = self.ema if self.ema is not None and not getattr(self.opt, "refreshes_engine", False) else None
        if self.norm is not None:
            self.last_grad_sumsq = self.norm.total()
            if getattr(self.opt, "refreshes_engine", False):          # FusedAdamW: the scale rides in the update launch
                self.opt.step(grad_sumsq=self.last_grad_sumsq, max_grad_norm=self.max_grad_norm)
            else:                                                      # torch.nn.utils.clip_grad_norm_ on the flat buffer (the .grad views)
                # a non-finite norm (overflow / NaN upstream): the update is skipped, as FusedAdamW's launch and the reference's GradScaler
                # do -- a NaN coefficient multiplied into the gradients would corrupt every parameter (one host read: this branch is not
                # the no-sync path)
                if bool(torch.isfinite(self.last_grad_sumsq).all()):
                    coef = (self.max_grad_norm / (self.last_grad_sumsq.sqrt() + 1e-6)).clamp(max=1.0)
                    self.fg.flat.mul_(coef)
                    self.opt.step()
                    if ema_after is not None:
                        ema_after.update(m)
        else:
            self.opt.step()
            if ema_after is not None:
                ema_after.update(m)
        # weights changed: the engine's bf16 / transposed copies have to follow.  dgs_amd.optim.FusedAdamW writes them in the same launch
        # as the update; for any other optimizer they are refreshed EXPLICITLY -- DGSDenoiser.engine() only notices parameter version
        # counters, and an optimizer is free not to move them (foreach / fused implementations, `p.data` updates, EMA swaps)
        if getattr(self.opt, "refreshes_engine", False):
            m.engine()
        else:
            m.refresh_engine_weights()
        return total / K

    # ---- the reference's training objective from a clean batch (PointDiffusionSystem.forward + training_step) ----
    LOSS_KEYS = ("lambda_diffusion", "lambda_lpips", "lambda_ssim", "lambda_pointsdist", "lambda_xyz")

    def configure_objective(self, diffusion, loss, perceptual=None):
        """diffusion: `dgs_amd.sampler.create_diffusion("1000")` (the reference's `diffusion_training`).
        loss: a mapping with the reference's `system.loss` keys -- lambda_diffusion, lambda_lpips, lambda_ssim, lambda_pointsdist,
        lambda_xyz -- each a number, a schedule list `[start_step, start_value, end_value, end_step]` (losses.scheduled_weight) or
        None / absent.  None or absent: the term is neither evaluated nor logged.  A number, 0.0 included, is evaluated, logged in
        `last_terms` and enters the sum with its weight, as in the reference.  lambda_depth must be 0 / None / absent: the reference's
        depth loss is commented out (utils/losses.py:294-297).
        perceptual: any callable (x, y) -> tensor on [n, 3, 256, 256] images in (-1, 1), on the model's device:
        `dgs_amd.lpips.LPIPS(net="vgg", weights=..., differentiable=True)` (HIP forward and input gradient in one call, memory bounded
        by its chunk) or the `lpips` package's frozen module.  It sees `losses.lpips_input(rendered)` and `losses.lpips_input(target)`
        (the HIP resize), loss_lpips is its `.mean()` (utils/losses.py:304-309) and its gradient reaches the renders through autograd.
        The library ships no weights."""
        loss = dict(loss)
        if loss.get("lambda_depth") not in (None, 0, 0.0):
            raise ValueError("lambda_depth: the reference's depth loss is commented out (utils/losses.py:294-297); there is no such term")
        unknown = sorted(k for k in loss if k.startswith("lambda_") and k not in self.LOSS_KEYS + ("lambda_depth",))
        if unknown:
            raise ValueError(f"unknown loss terms {unknown}; the reference has {list(self.LOSS_KEYS)}")
        lam = {k: loss.get(k) for k in self.LOSS_KEYS}
        for k, v in lam.items():
            if v is not None:
                losses.scheduled_weight(v, 0)                                  # a TypeError now, not at step 0
        if lam["lambda_lpips"] is not None and perceptual is None:
            raise ValueError("lambda_lpips is set: pass the network as `perceptual` (e.g. lpips.LPIPS(net='vgg')); this library has none")
        if all(v is None for v in lam.values()):
            raise ValueError("configure_objective: every loss term is None")
        if diffusion.num_timesteps != 1000:
            raise ValueError(f"the reference trains on create_diffusion('1000'); this one has {diffusion.num_timesteps} steps")
        self._objective = (diffusion, lam, perceptual)

    def train_step(self, batch, noise=None, timesteps=None):
        """PointDiffusionSystem.forward + training_step (systems/diffusion_gs_system.py:71-129) on the reference's CLEAN batch -- keys
        rgbs_input, c2ws_input, fxfycxcys_input, depths_input, masks_input (the input views) and c2ws, fxfycxcys, rgbs, masks (all
        rendered views) -- after `configure_objective`:
            noise = randn_like(rgbs_input), then timesteps = randint(0, T, (b,)), on the batch's device: from one torch.manual_seed
                the reference's draws (pass either to override)
            rays of the input views                                             HIP: backend.rays_from_c2w
            noisy views + gt_img_aligned_xyz = ray_o + ray_d * depths_input     HIP: ONE launch, diffusion.training_inputs
            per micro-batch: forward, render, image terms (losses.image_losses / mse_psnr), point terms on `aligned`
                (losses.points_losses), the perceptual slot; loss = sum_k scheduled_weight(lambda_k, global_step) * loss_k
            the scaling, all-reduce, clip, optimizer step, EMA and refresh of `step` (the same loop)
        The noisy views go into a fresh tensor: the caller's batch is NOT modified (the reference noises `batch['rgbs_input']` in place).
        loss_xyz is one scalar for the local batch, sum / masks_input.sum(): a micro-batch divides its sum by the WHOLE local batch's
        mask sum, on the device, so the gradient is that of the unsplit evaluation.  Afterwards `last_terms` holds what the reference
        logs under train/ and train_params/ (detached device scalars `loss_*`, the weights used `lambda_*`) and what its forward returns
        besides (`timesteps`, `x_t`, the weighted `loss`); `global_step` has advanced by one and
        `diffusion.bad_t` is still 0 unless a given timestep was outside [0, T).  Returns the (local) weighted loss."""
        if self._objective is None:
            raise RuntimeError("DataParallelTrainer.train_step before configure_objective")
        self._check_open()
        diffusion, lam, perceptual = self._objective
        m = self.model
        lib = getattr(m, "_lib", None)
        clean = batch["rgbs_input"]
        b, _v, _c, H, W = clean.shape
        if noise is None:
            noise = torch.randn_like(clean)                                     # :77
        if timesteps is None:
            timesteps = torch.randint(0, diffusion.num_timesteps, (b,), device=clean.device)     # :79-85
        timesteps = timesteps.long()
        ray_o, ray_d = self._raster_backend.rays_from_c2w(batch["c2ws_input"], batch["fxfycxcys_input"], H, W)
        want_xyz = lam["lambda_xyz"] is not None
        x_t, gt_xyz = diffusion.training_inputs(clean, timesteps, noise, *((batch["depths_input"], ray_o, ray_d) if want_xyz else ()))
        masks_in = batch["masks_input"].float() if want_xyz else None
        mask_sum = masks_in.sum(dtype=torch.float64).float().reshape(1) if want_xyz else None      # stays on the device
        w = {k: (None if v is None else float(losses.scheduled_weight(v, self.global_step, self.epoch))) for k, v in lam.items()}
        target = batch["rgbs"]
        sums = {}

        def add(name, value):
            sums[name] = sums[name] + value.detach() if name in sums else value.detach()

        def micro_loss(sl, rendered, aligned, K):
            tgt = target[sl].to(rendered.dtype)
            parts = []
            if w["lambda_ssim"] is not None:                                   # one fused node for both image terms, as in `step`
                img, l2, self.last_psnr, ssim_term = losses.image_losses(rendered, tgt, w["lambda_diffusion"] or 0.0, w["lambda_ssim"], lib=lib)
                self.last_ssim_loss = ssim_term.detach()
                add("loss_ssim", ssim_term.mean())
                if w["lambda_diffusion"] is not None:
                    add("loss_diffusion", l2.mean())
                parts.append(img)
            elif w["lambda_diffusion"] is not None:
                mse, _l2, self.last_psnr = losses.mse_psnr(rendered, tgt, lib=lib)
                add("loss_diffusion", mse)
                parts.append(mse * w["lambda_diffusion"])                    # weight 1.0: the bits of `step`
            if want_xyz:
                pd, xyz = losses.points_losses_part(aligned, ray_o[sl], gt_xyz[sl], masks_in[sl], mask_sum, lib=lib)
                xyz = xyz * float(K)                   # the parts ADD up to the batch's scalar; the loop takes the MEAN over micro-batches
                add("loss_xyz", xyz)
                parts.append(xyz * w["lambda_xyz"])
            elif w["lambda_pointsdist"] is not None:
                pd, _ = losses.points_losses(aligned, ray_o[sl], lib=lib)
            if w["lambda_pointsdist"] is not None:
                pd = pd.mean()                                               # the system's `pointsdist_loss.mean()`, :109
                add("loss_pointsdist", pd)
                parts.append(pd * w["lambda_pointsdist"])
            if w["lambda_lpips"] is not None:
                flat = lambda x: x.reshape(-1, *x.shape[2:])
                lp = perceptual(losses.lpips_input(flat(rendered), lib=lib), losses.lpips_input(flat(tgt), lib=lib)).mean()
                add("loss_lpips", lp)
                parts.append(lp * w["lambda_lpips"])
            loss = parts[0]
            for p in parts[1:]:
                loss = loss + p
            return loss

        total = self._optimizer_step(x_t, ray_o, ray_d, timesteps, batch["c2ws"], batch["fxfycxcys"], micro_loss)
        self.last_terms = {k: v / self._micro_batches for k, v in sums.items()}
        self.last_terms.update({k: v for k, v in w.items() if v is not None})
        self.last_terms.update(timesteps=timesteps, x_t=x_t, loss=total)
        self.global_step += 1
        return total
