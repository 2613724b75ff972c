"""FusedSGD / FusedAdam: torch.optim.SGD / Adam semantics in three HIP launches over ALL parameter tensors (pts/solver.hip).

The reference's step is ``zero_grad -> backward -> clip_grad_norm_ -> optimizer.step() -> scheduler.step()`` (engine/trainer.py:110-115)
with torch.optim.SGD(momentum) or Adam from solver/build.py.  torch's own step is a chain of multi-tensor launches and, for SGD, bakes the
learning rate into a captured graph as a kernel argument.  Here

  * ``param_groups`` stays the host truth with torch's keys, so ``_LRScheduler`` and ``OneCycleScheduler`` drive it unchanged;
  * the values the kernels use live in a small device table (``push_hyper()``: one host-to-device copy when a group value changed), so a
    captured step replays with whatever was pushed last:   ``scheduler.step(); opt.push_hyper(); graphed()``;
  * parameters and gradients are reached through a device table of their own pointers (refreshed when a pointer changed), so gradients
    that are views of ``comm.GradientSync``'s flat buffer need no packing, and nothing needs a particular alignment;
  * the state lives in flat fp32 buffers and is exposed per parameter in ``self.state[p]`` under torch's names as views, so
    ``state_dict()`` / ``load_state_dict()`` interchange with torch.optim checkpoints.

There is no CPU path: ``step()`` on CPU parameters raises.  Under stream capture ``step()`` uploads nothing; a table that would have to
change raises.  One difference from torch: Adam's bias correction uses ONE step count for all parameters (the device counter), where
torch counts per parameter; they differ only for a parameter that is without a gradient in some steps.
"""
import torch
from torch.optim import Optimizer

TENSOR_COLS, CHUNK_COLS, HYPER_COLS, DERIVED_COLS = 5, 2, 8, 2
FLAG_NORM, FLAG_KEEP_COEF, FLAG_ADVANCE = 1, 2, 4
_CAPTURE_HELP = ("call zero_grad() / GradientSync.zero_grad() (so that every gradient exists and stays where it is) and push_hyper() "
                 "before capturing")


def state_offsets(numels):
    """Offset of every parameter in the flat state buffers (floats): parameter order, each start rounded up to 4 floats so that the
    kernels' 16-byte accesses to the state are aligned.  -> (offsets, total)"""
    offs, off = [], 0
    for n in numels:
        offs.append(off)
        off += (int(n) + 3) // 4 * 4
    return offs, off


def chunk_table(numels, has_grad, chunk):
    """The per-chunk half of the work table: [(tensor index, start)] in tensor order, then ascending start.  A tensor without a gradient or
    without elements has no chunk."""
    out = []
    for i, (n, g) in enumerate(zip(numels, has_grad)):
        if g:
            out.extend((i, s) for s in range(0, int(n), chunk))
    return out


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class _FusedOptimizer(Optimizer):
    _ADAM = False
    _STATE_NAMES = ()

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        for p in self._params():
            if p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                raise ValueError(f"{type(self).__name__} takes contiguous fp32 parameters, got {p.dtype} "
                                 f"{'contiguous' if p.is_contiguous() else 'non-contiguous'} of shape {tuple(p.shape)}")
        self._flat = None               # {state name: flat fp32 buffer}
        self._dev = None                # device tables: tensors, chunks, partials, hyper, derived, scalars, step
        self._ptr_key = None
        self._hyper_key = None
        self._n_chunks = 0
        self._armed = False             # clip_grad_norm_ ran: the next step() clips with the coefficient it left on the device
        self._step_host = 0             # the count to start the device counter from (load_state_dict)
        self._constructed = True

    def add_param_group(self, param_group):
        """Groups are fixed at construction: the flat state buffers and the device tables are laid out for them."""
        if getattr(self, "_constructed", False):
            raise NotImplementedError(f"{type(self).__name__}: add_param_group() after construction is not built (the flat state buffers "
                                      "are laid out once); build the optimizer with all its groups")
        super().add_param_group(param_group)

    # ---- layout
    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _layout(self):
        params, groups = [], []
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                params.append(p)
                groups.append(gi)
        return params, groups

    def _device(self):
        params = self._params()
        devs = {p.device for p in params}
        if len(devs) != 1:
            raise RuntimeError(f"{type(self).__name__}: the parameters must be on one device, got {sorted(map(str, devs))}")
        return devs.pop()

    def _uses_state(self):
        return True

    def _ensure_flat(self, device):
        """The flat state buffers, zero-initialised, on the parameters' device."""
        if self._flat is None or any(b.device != device for b in self._flat.values()):
            _, total = state_offsets([p.numel() for p in self._params()])
            self._flat = {n: torch.zeros(total, dtype=torch.float32, device=device) for n in self._STATE_NAMES}
        return self._flat

    def _ensure_scalars(self, device):
        if self._dev is None or self._dev["scalars"].device != device:
            self._dev = {"scalars": torch.zeros(4, dtype=torch.float32, device=device),
                         "step": torch.full((1,), int(self._step_host), dtype=torch.int64, device=device)}
            self._dev["scalars"][1] = 1.0
            self._dev["scalars"][2] = float(self._step_host)
            self._ptr_key = self._hyper_key = None
        return self._dev

    def _state_views(self, p, off):
        n = p.numel()
        return {name: self._flat[name][off:off + n].view_as(p) for name in self._STATE_NAMES}

    def _attach_state(self, p, off):
        self.state[p].update(self._state_views(p, off))

    # ---- hyper table
    def _hyper_row(self, group):
        raise NotImplementedError

    def _hyper_rows(self):
        return tuple(self._hyper_row(g) for g in self.param_groups)

    def push_hyper(self):
        """Copy the groups' values (lr, weight decay, momentum / betas, eps) to the device if one changed: call it after a scheduler step
        and before replaying a captured step."""
        rows = self._hyper_rows()
        if rows == self._hyper_key and self._dev is not None and "hyper" in self._dev:
            return
        if _capturing():
            raise RuntimeError(f"{type(self).__name__}: a group's lr / weight decay / momentum changed under stream capture, where nothing "
                               f"is uploaded: {_CAPTURE_HELP}")
        device = self._device()
        if device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only (parameters on {device}); there is no CPU fallback")
        dev = self._ensure_scalars(device)
        host = torch.tensor(rows, dtype=torch.float32).reshape(len(rows), HYPER_COLS)
        if "hyper" not in dev or dev["hyper"].shape != host.shape:
            dev["hyper"] = torch.empty_like(host, device=device)
            dev["derived"] = torch.zeros(len(rows), DERIVED_COLS, dtype=torch.float32, device=device)
        dev["hyper"].copy_(host)
        self._hyper_key = rows

    # ---- pointer table
    def _refresh_tables(self):
        params, groups = self._layout()
        key = tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for p in params)
        if key == self._ptr_key and (self._flat is not None or not self._uses_state()):
            return
        if _capturing():
            raise RuntimeError(f"{type(self).__name__}: a parameter or gradient pointer changed under stream capture, where the device "
                               f"table cannot be refreshed: {_CAPTURE_HELP}")
        device = self._device()
        if device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only (parameters on {device}); there is no CPU fallback")
        for p in params:
            g = p.grad
            if g is None:
                continue
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.device != device or g.shape != p.shape:
                raise RuntimeError(f"{type(self).__name__}: gradients must be contiguous fp32 on {device} with the parameter's shape "
                                   f"(got {g.dtype} {tuple(g.shape)} on {g.device})")
        from ..pts import _lib
        chunk = _lib.lib().drc_solver_chunk()
        numels = [p.numel() for p in params]
        offs, _ = state_offsets(numels)
        has_grad = [p.grad is not None for p in params]
        chunks = chunk_table(numels, has_grad, chunk)
        dev = self._ensure_scalars(device)
        if self._uses_state():
            self._ensure_flat(device)
            for p, off, g in zip(params, offs, has_grad):
                if g and not all(n in self.state[p] for n in self._STATE_NAMES):
                    self._attach_state(p, off)
        rows = [[kp, kg, off, n, gi] for (kp, kg), off, n, gi in zip(key, offs, numels, groups)]
        dev["tensors"] = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), TENSOR_COLS).to(device)
        dev["chunks"] = torch.tensor(chunks, dtype=torch.int64).reshape(len(chunks), CHUNK_COLS).to(device)
        if "partials" not in dev or dev["partials"].numel() < len(chunks):
            dev["partials"] = torch.zeros(max(len(chunks), 1), dtype=torch.float64, device=device)
        self._n_chunks, self._n_tensors = len(chunks), len(rows)
        self._updated = [p for p, g in zip(params, has_grad) if g and p.numel()]
        self._ptr_key = key

    # ---- launches
    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()

    def _launch_norm(self, L, stream):
        from ..pts import _lib
        d = self._dev
        _lib.check(L.drc_solver_grad_norm(self._n_chunks, self._n_tensors, d["tensors"].data_ptr(), d["chunks"].data_ptr(),
                                          d["partials"].data_ptr(), stream), "drc_solver_grad_norm")

    def _launch_prepare(self, L, stream, flags, max_norm):
        from ..pts import _lib
        d = self._dev
        _lib.check(L.drc_solver_prepare(self._n_chunks, d["partials"].data_ptr(), flags, float(max_norm), len(self.param_groups),
                                        int(self._ADAM), d["hyper"].data_ptr(), d["derived"].data_ptr(), d["scalars"].data_ptr(),
                                        d["step"].data_ptr(), stream), "drc_solver_prepare")

    def _launch_step(self, L, stream, clip):
        raise NotImplementedError

    def _begin(self):
        from ..pts import _lib
        self._refresh_tables()
        self.push_hyper()
        return _lib.lib(), torch.cuda.current_stream().cuda_stream

    @staticmethod
    def _check_max_norm(max_norm):
        max_norm = float(max_norm)
        if not max_norm >= 0.0:
            raise ValueError(f"max_norm must be >= 0, got {max_norm}")
        return max_norm

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm, norm_type=2.0):
        """torch.nn.utils.clip_grad_norm_ over this optimizer's parameters: computes the 2-norm of all gradients now and arms the clip for
        the next ``step()``, which scales the gradients (and writes them back scaled) as it reads them.  Returns the device scalar
        ``total_norm`` without a host sync; it is a view that the next norm overwrites."""
        if float(norm_type) != 2.0:
            raise NotImplementedError("only the 2-norm is built")
        max_norm = self._check_max_norm(max_norm)
        L, stream = self._begin()
        self._launch_norm(L, stream)
        self._launch_prepare(L, stream, FLAG_NORM, max_norm)
        self._armed = True
        return self._dev["scalars"][0]

    @property
    def total_norm(self):
        """The device scalar the last norm was written to."""
        return None if self._dev is None else self._dev["scalars"][0]

    def step(self, closure=None, max_norm=None):
        """One update of every parameter that has a gradient.  ``max_norm``: clip the gradients' total 2-norm to it first (three launches:
        norm, prepare, step); None does not clip unless ``clip_grad_norm_`` armed it."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        with torch.no_grad():
            L, stream = self._begin()
            if max_norm is not None:
                max_norm = self._check_max_norm(max_norm)
                self._launch_norm(L, stream)
                self._launch_prepare(L, stream, FLAG_NORM | FLAG_ADVANCE, max_norm)
                clip = True
            elif self._armed:
                self._launch_prepare(L, stream, FLAG_KEEP_COEF | FLAG_ADVANCE, 0.0)
                clip = True
            else:
                self._launch_prepare(L, stream, FLAG_ADVANCE, 0.0)
                clip = False
            self._armed = False
            self._launch_step(L, stream, clip)
            self.bump_versions()
        return loss

    def bump_versions(self):
        """The kernels write the weights through raw pointers: tell autograd and every ``_version``-keyed cache (the folded layers of
        pytorch_utils, head_ops) that they changed.  ``step()`` does it; call it yourself after REPLAYING a captured step."""
        if getattr(self, "_updated", None):
            torch.autograd.graph.increment_version(self._updated)

    # ---- gradients
    @torch.no_grad()
    def zero_grad(self, set_to_none=False):
        """Zero the gradients IN PLACE (they keep their addresses, as a captured step needs): one memset when they are views that tile one
        flat buffer (comm.GradientSync.zero_grad()), one multi-tensor launch otherwise.  ``set_to_none=True`` is torch's."""
        if set_to_none:
            return super().zero_grad(set_to_none=True)
        grads = [p.grad for p in self._params() if p.grad is not None]
        if not grads:
            return
        for g in grads:
            if g.grad_fn is not None:
                g.detach_()
            else:
                g.requires_grad_(False)
        g0 = grads[0]
        base = g0.untyped_storage().data_ptr()
        if all(g.dtype == torch.float32 and g.is_contiguous() and g.device == g0.device and g.untyped_storage().data_ptr() == base
               for g in grads):
            spans = sorted((g.data_ptr(), g.numel() * 4) for g in grads if g.numel())
            end = lo = spans[0][0] if spans else base
            for a, n in spans:
                if a != end:
                    break
                end = a + n
            else:
                if end > lo:
                    torch.empty(0, dtype=torch.float32, device=g0.device).set_(g0.untyped_storage(), (lo - base) // 4,
                                                                               ((end - lo) // 4,)).zero_()
                return
        torch._foreach_zero_(grads)

    # ---- checkpoints
    def _read_step(self, values):
        return 0

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """torch's, then the loaded per-parameter tensors move into the flat buffers (``self.state[p]`` holds views again)."""
        super().load_state_dict(state_dict)
        params = self._params()
        if not params:
            return
        device = self._device()
        offs, _ = state_offsets([p.numel() for p in params])
        self._flat = None
        loaded = {p: dict(self.state[p]) for p in params if p in self.state and self.state[p]}
        steps = []
        if self._uses_state() or any(any(n in s for n in self._STATE_NAMES) for s in loaded.values()):
            self._ensure_flat(device)
            for p, off in zip(params, offs):
                s = loaded.get(p)
                if not s:
                    continue
                views = self._state_views(p, off)
                for name, v in views.items():
                    if name in s and s[name] is not None:
                        v.copy_(s[name])
                self.state[p].update(views)
                if "step" in s:
                    steps.append(s["step"])
        self._step_host = self._read_step(steps)
        if self._dev is not None and self._dev["scalars"].device == device:
            self._dev["step"].fill_(int(self._step_host))
            self._dev["scalars"][2] = float(self._step_host)
        for p in params:
            if p in loaded and "step" in loaded[p]:
                self.state[p]["step"] = self._step_view(device)
        self._ptr_key = self._hyper_key = None
        self._armed = False

    def _step_view(self, device):
        return None


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD(params, lr, momentum, weight_decay) -- dampening 0, no Nesterov -- as one HIP launch over all tensors.

    One difference from torch where groups MIX zero and non-zero momentum: as soon as any group has momentum != 0, every parameter with a
    gradient gets a `momentum_buffer` (the one flat buffer serves all tensors; with momentum 0 it holds the last decayed gradient and
    does not enter the update), where torch keeps none for the momentum-0 groups.  torch loads such a `state_dict()` all the same.  With
    momentum 0 in every group there is no buffer and no state, as in torch."""
    _STATE_NAMES = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f"invalid lr / momentum / weight_decay: {lr} / {momentum} / {weight_decay}")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize,
                        foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults)
        self._hyper_rows()              # refuses what is not built

    def _uses_state(self):
        # torch keeps a momentum buffer only where momentum != 0
        return self._flat is not None or any(float(g["momentum"]) != 0.0 for g in self.param_groups)

    def _hyper_row(self, g):
        if g.get("nesterov") or float(g.get("dampening", 0.0)) != 0.0 or g.get("maximize"):
            raise NotImplementedError("FusedSGD: nesterov, dampening != 0 and maximize are not built")
        mu = float(g["momentum"])
        if mu < 0.0:
            raise ValueError(f"momentum must be >= 0, got {mu}")
        return (float(g["lr"]), float(g["weight_decay"]), mu, 0.0, 0.0, 0.0, 0.0, 0.0)

    def _launch_step(self, L, stream, clip):
        from ..pts import _lib
        d = self._dev
        buf = self._flat["momentum_buffer"] if self._flat is not None else None
        _lib.check(L.drc_solver_sgd_step(self._n_chunks, self._n_tensors, len(self.param_groups), d["tensors"].data_ptr(),
                                         d["chunks"].data_ptr(), d["hyper"].data_ptr(), d["scalars"].data_ptr(), self._ptr(buf),
                                         int(clip), stream), "drc_solver_sgd_step")


class FusedAdam(_FusedOptimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) -- L2 weight decay on the gradient, no amsgrad -- as one HIP launch."""
    _ADAM = True
    _STATE_NAMES = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, maximize=False):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid lr / betas / eps / weight_decay: {lr} / {betas} / {eps} / {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self._hyper_rows()

    def _hyper_row(self, g):
        if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay"):
            raise NotImplementedError("FusedAdam: amsgrad, maximize and decoupled weight decay (AdamW) are not built")
        b1, b2 = (float(b) for b in g["betas"])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must be in [0, 1), got {(b1, b2)}")
        # the complements travel rounded from the doubles: 1 - float32(0.999) is 1.3e-5 off its value
        return (float(g["lr"]), float(g["weight_decay"]), b1, b2, float(g["eps"]), 1.0 - b1, 1.0 - b2, 0.0)

    def _attach_state(self, p, off):
        super()._attach_state(p, off)
        self.state[p]["step"] = self._step_view(p.device)

    def _step_view(self, device):
        """state['step']: torch keeps a float scalar per parameter; here every parameter sees the one device count."""
        return self._ensure_scalars(device)["scalars"][2] if device.type == "cuda" else torch.tensor(float(self._step_host))

    def state_dict(self):
        """torch's, with `step` as torch.optim.Adam keeps it: an independent fp32 CPU scalar per parameter.  In `self.state` every
        parameter sees the ONE device count; handed out like that, torch's Adam -- which keeps loaded `step` tensors as they are and
        increments each parameter's in place -- would advance a shared count once per parameter.  One host read of the count."""
        sd = super().state_dict()
        if any("step" in s for s in sd["state"].values()):
            count = self._step_host if self._dev is None else float(self._dev["scalars"][2])
            sd["state"] = {i: ({**s, "step": torch.tensor(float(count), dtype=torch.float32)} if "step" in s else s)
                           for i, s in sd["state"].items()}
        return sd

    def _read_step(self, values):
        steps = {int(float(v)) for v in values}
        if len(steps) > 1:
            raise ValueError(f"FusedAdam keeps one step count for all parameters; the checkpoint has {sorted(steps)}")
        return steps.pop() if steps else 0

    def _launch_step(self, L, stream, clip):
        from ..pts import _lib
        d = self._dev
        _lib.check(L.drc_solver_adam_step(self._n_chunks, self._n_tensors, len(self.param_groups), d["tensors"].data_ptr(),
                                          d["chunks"].data_ptr(), d["hyper"].data_ptr(), d["derived"].data_ptr(),
                                          d["scalars"].data_ptr(), self._flat["exp_avg"].data_ptr(),
                                          self._flat["exp_avg_sq"].data_ptr(), int(clip), stream), "drc_solver_adam_step")
