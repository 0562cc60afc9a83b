"""The optimisers the reference trains its slide classifier with (conf/model/optim/), and the training step that stays on
the device.

`Lamb` and `SAM` mirror vq_ae/optim/lamb.py and vq_ae/optim/sam.py as plain `torch.optim.Optimizer`s: the same torch
operations in the same order on any parameters on any device, so in fp64 they retrace the reference's trajectories and in
fp32 they are the yardstick the HIP kernel is measured against.  `SAM` takes the base optimiser as a class, a factory
`f(param_groups, **overrides)` or the reference's `base_optimizer_conf` dict, whose `_target_` is resolved by import path
(no hydra; `vq_ae.optim.lamb.Lamb` resolves to the mirror here).

`FusedAdam`, `FusedAdamW` and `FusedLamb` are the same optimisers for any parameter list -- the ~1 600 tensors of an Encoder /
Decoder -- as `torch.optim.Optimizer`s whose device step is csrc/optim.hip: one launch (Adam / AdamW) or three (LAMB, SAM's
climb) over all tensors, the per-tensor norms and SAM's global norm formed on the device, nothing read back.  `SAM` accepts
them as base optimiser (class, factory or `_target_: vqae_amd.optim.FusedLamb`) and then climbs and restores in the same
handle.  On CPU tensors they run `Lamb` / torch's Adam and AdamW; their state_dict is torch.optim's either way.

`ClassifierTrainer` is one training step of `loss_and_grads` + `optimizer.step()` without the host in between: it owns a
vqae_classifier made from the module's parameters and a vqae_classifier_optim on it (csrc/classifier_optim.hip); `step` runs
vqae_classifier_loss_grad and the optimiser kernel on the packed gradient in HBM, which rewrites the weight image the next
loss_grad reads, and returns the loss and the stats rows as device tensors without synchronising.  With `sam_rho` it is
CNNClassifier.sam_step_and_update (validation_nn/model.py:115-129): loss_grad, climb, loss_grad at the climbed weights,
restore + base step.  On CPU tensors the same class runs the torch restatement (torch_loss_grad and the mirrors).  Its
state_dict has torch.optim's layout, so a run moves between the trainer and torch.optim.AdamW or `Lamb` either way."""
import copy
import ctypes
import importlib

import numpy as np
import torch
from torch.optim import Optimizer

from . import _lib as L
from . import ops
from .classifier import NativeClassifier, _as_codes, _check_codes, ce_arguments
from .classifier_train import PARAM_NAMES, _as_labels, _params, ce_weight_sum, torch_ce_loss_grad, torch_loss_grad


class Lamb(Optimizer):
    """vq_ae.optim.lamb.Lamb: Adam's moments and bias corrections, the step of each tensor scaled by its trust ratio
    ||p|| / ||step|| (1 where either norm is 0)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        for i in (0, 1):
            if not 0.0 <= betas[i] < 1.0:
                raise ValueError(f"Invalid beta parameter at index {i}: {betas[i]}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad.data
                if g.is_sparse:
                    raise RuntimeError("Lamb does not support sparse gradients")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p.data)
                    st["exp_avg_sq"] = torch.zeros_like(p.data)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                st["step"] += 1
                m.mul_(b1).add_(g, alpha=1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                bc1, bc2 = 1 - b1 ** st["step"], 1 - b2 ** st["step"]
                u = (m / bc1) / ((v / bc2).sqrt() + group["eps"])
                if group["weight_decay"] != 0:
                    u.add_(p.data, alpha=group["weight_decay"])
                wn, un = torch.norm(p.data), torch.norm(u)
                trust = wn / un if wn > 0 and un > 0 else 1.0
                p.data.add_(u, alpha=-group["lr"] * trust)
        return loss


# ---- the fused multi-tensor step (csrc/optim.hip) ----------------------------------------------------------------------------
def _dense(t):
    """Dense and non-overlapping in any memory format: walking the storage visits every element once."""
    n = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda x: x[1]):
        if stride != n:
            return False
        n *= size
    return True


def _storage_order(t, like):
    """`t` (the logical shape of `like`) as a flat view of its elements in the order `like` keeps them in memory."""
    if t.stride() != like.stride():
        t = torch.empty_like(like, dtype=t.dtype, device=t.device).copy_(t)
    return t.as_strided((t.numel(),), (1,), t.storage_offset())


class _Fused(Optimizer):
    """What FusedAdam, FusedAdamW and FusedLamb share.  On device parameters a step collects the parameter and gradient
    addresses and calls vqae_optim_step on the current stream: nothing is read back, the moments live dense in a
    vqae_optim handle and come out as tensors only for state_dict().  On CPU parameters the step is the torch code of
    `_cpu_class` on this optimiser's own param_groups and state.  Either way state_dict() has torch.optim's layout."""
    _kind = None
    _cpu_class = None

    def __init__(self, params, defaults):
        self._h = None                  # the vqae_optim handle, its parameters and the address arrays of a step
        self._sig = None
        self._params = []
        self._cpu = None
        self._climbing = False          # a SAM first step is waiting for its step
        super().__init__(params, defaults)

    # ---- parameters ---------------------------------------------------------------------------------------------------------
    def _all_params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def add_param_group(self, param_group):
        """After the first device step this rebuilds the handle at the next step; the state is kept."""
        if getattr(self, "_h", None) is not None:
            self._export_into_state()
            self._drop()
        super().add_param_group(param_group)
        ps = self._all_params()
        for p in ps:
            if p.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"{type(self).__name__} steps fp32 parameters (fp64 on the CPU), got {p.dtype}")
        if len({p.device for p in ps}) > 1:
            raise ValueError(f"{type(self).__name__}: the parameters are on several devices: "
                             f"{sorted(str(p.device) for p in ps)[0]} ... {sorted(str(p.device) for p in ps)[-1]}")

    def _on_device(self):
        return self.param_groups[0]["params"][0].is_cuda

    def _configs(self):
        arr = (L.ClassifierOptimConfig * len(self.param_groups))()
        for k, g in enumerate(self.param_groups):
            for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
                if g.get(flag):
                    raise NotImplementedError(f"{type(self).__name__}: {flag}=True is not provided")
            rho = g.get("rho")
            arr[k] = L.ClassifierOptimConfig(L.OPTIM_KINDS[self._kind], float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]),
                                             float(g["eps"]), float(g["weight_decay"]), -1.0 if rho is None else float(rho),
                                             int(bool(g.get("adaptive", False))))
        return arr

    # ---- the handle ---------------------------------------------------------------------------------------------------------
    def _ensure_handle(self):
        params = self._all_params()
        sig = tuple(map(id, params))
        if self._h is not None and sig == self._sig:
            return
        if self._h is not None:                                   # the parameter list changed under a live handle
            self._export_into_state()
            self._drop()
        group_of = [k for k, g in enumerate(self.param_groups) for _ in g["params"]]
        for p in params:
            if p.dtype != torch.float32:
                raise TypeError(f"{type(self).__name__} steps fp32 parameters on the device, got {p.dtype}")
            if p.device != params[0].device:
                raise ValueError(f"{type(self).__name__}: the parameters are on several devices")
            if p.numel() < 1 or not _dense(p):
                raise ValueError(f"{type(self).__name__}: a parameter of shape {tuple(p.shape)} and strides {p.stride()} is empty or "
                                 "not dense in memory")
        n = len(params)
        numel = (ctypes.c_int64 * n)(*[p.numel() for p in params])
        h = ctypes.c_void_p()
        cfgs = self._configs()
        with torch.cuda.device(params[0].device):
            L.check(L.lib().vqae_optim_create(n, numel, (ctypes.c_int * n)(*group_of), len(self.param_groups), cfgs, ctypes.byref(h)))
        self._h, self._sig, self._params = h, sig, params
        self._strides = [p.stride() for p in params]
        self._pp, self._gp = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
        if self.state:
            self._import_from_state()
            self.state.clear()

    def _drop(self):
        if getattr(self, "_h", None) is not None:
            if self._climbing:
                raise RuntimeError(f"{type(self).__name__}: a SAM first step is waiting for its second step")
            L.lib().vqae_optim_destroy(self._h)
        self._h, self._sig, self._params = None, None, []

    def __del__(self):
        try:
            if self._h is not None:
                L.lib().vqae_optim_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _step_value(self, k):
        return int(k) if self._kind == "lamb" else torch.tensor(float(k), dtype=torch.float32)

    def _export_into_state(self):
        """The handle's moments and step counts as self.state entries (tensors on the parameters' device, of their shapes and
        strides; a tensor that has not stepped has no entry, as in torch's lazy state).  Synchronises."""
        params = self._params
        total = sum(p.numel() for p in params)
        m, v = np.empty(total, np.float32), np.empty(total, np.float32)
        steps = (ctypes.c_int64 * len(params))()
        dev = params[0].device
        with torch.cuda.device(dev):
            L.check(L.lib().vqae_optim_export(self._h, m.ctypes.data, v.ctypes.data, steps, ops._stream()))
            m, v = torch.from_numpy(m).to(dev), torch.from_numpy(v).to(dev)
        o = 0
        for p, k in zip(params, steps):
            n = p.numel()
            if k > 0:
                self.state[p] = {"step": self._step_value(k), "exp_avg": m[o:o + n].as_strided(p.shape, p.stride()),
                                 "exp_avg_sq": v[o:o + n].as_strided(p.shape, p.stride())}
            o += n

    def _import_from_state(self):
        params = self._params
        total = sum(p.numel() for p in params)
        m, v = np.zeros(total, np.float32), np.zeros(total, np.float32)
        steps = (ctypes.c_int64 * len(params))()
        o = 0
        for i, p in enumerate(params):
            n = p.numel()
            st = self.state.get(p)
            if st:
                steps[i] = int(st["step"])
                for dst, key in ((m, "exp_avg"), (v, "exp_avg_sq")):
                    t = st[key]
                    if tuple(t.shape) != tuple(p.shape):
                        raise ValueError(f"{type(self).__name__}: {key} of shape {tuple(t.shape)} for a parameter of shape {tuple(p.shape)}")
                    dst[o:o + n] = _storage_order(t.detach().to(torch.float32), p).cpu().numpy()
            o += n
        with torch.cuda.device(params[0].device):
            L.check(L.lib().vqae_optim_import(self._h, m.ctypes.data, v.ctypes.data, steps, ops._stream()))

    # ---- the step -----------------------------------------------------------------------------------------------------------
    def _run(self, first):
        self._ensure_handle()
        name = type(self).__name__
        pp, gp, keep = [], [], []
        for p, strides in zip(self._params, self._strides):        # (the host's share of a step: kept short)
            g = p.grad
            pp.append(p.data_ptr())
            if g is None:
                gp.append(None)
                continue
            if g.is_sparse:
                raise RuntimeError(f"{name} does not support sparse gradients")
            if g.stride() != strides:                              # (dtype and device are the parameter's: torch checks `.grad =`)
                g = torch.empty_like(p).copy_(g)                   # the parameter's layout
                keep.append(g)
            gp.append(g.data_ptr())
        self._pp[:] = pp
        self._gp[:] = gp
        lib = L.lib()
        with torch.cuda.device(self._params[0].device):
            L.check(lib.vqae_optim_set(self._h, self._configs()))   # the groups are read at every step: lr schedules
            L.check((lib.vqae_optim_sam_first if first else lib.vqae_optim_step)(self._h, self._pp, self._gp, ops._stream()))
        self._climbing = first

    def _cpu_opt(self):
        if self._cpu is None:
            d = self.defaults
            self._cpu = self._cpu_class(self.param_groups, lr=d["lr"], betas=d["betas"], eps=d["eps"], weight_decay=d["weight_decay"])
        self._cpu.param_groups, self._cpu.state = self.param_groups, self.state
        return self._cpu

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._on_device():
            self._run(False)
        else:
            self._configs()                                        # the same NotImplementedErrors on either path
            self._cpu_opt().step()
        return loss

    # ---- state --------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """torch.optim's layout: state[i] = {step, exp_avg, exp_avg_sq} of parameter i's shape (step as the installed torch's
        Adam / AdamW keeps it, an int for LAMB), what torch.optim.Adam / AdamW / `Lamb` load.  With a live handle this
        downloads the moments (one synchronising copy)."""
        live = self._h is not None
        if live:
            self._export_into_state()
        sd = super().state_dict()
        if live:
            self.state.clear()
        return sd

    def load_state_dict(self, state_dict):
        self._drop()                                               # the next device step builds a handle from the loaded state
        super().load_state_dict(state_dict)

    def __getstate__(self):                                        # copy.deepcopy and pickle: through the exported state
        live = self._h is not None
        if live:
            self._export_into_state()
        out = {"defaults": self.defaults, "state": dict(self.state), "param_groups": self.param_groups}
        if live:
            self.state.clear()
        return out

    def __setstate__(self, state):
        self._drop()
        self._cpu, self._climbing = None, False
        super().__setstate__(state)
        if not hasattr(self.state, "default_factory"):
            from collections import defaultdict
            self.state = defaultdict(dict, self.state)


def _check_hyper(lr, betas, eps, weight_decay):
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    for i in (0, 1):
        if not 0.0 <= betas[i] < 1.0:
            raise ValueError(f"Invalid beta parameter at index {i}: {betas[i]}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")


class FusedAdam(_Fused):
    """torch.optim.Adam (single-tensor form, amsgrad=False, maximize=False) with one fused launch per step on device
    parameters.  Constructor, defaults and ValueErrors are torch.optim.Adam's; amsgrad / maximize / capturable /
    differentiable raise NotImplementedError, foreach and fused are accepted and not read."""
    _kind = "adam"
    _cpu_class = torch.optim.Adam
    _weight_decay = 0.0

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None):
        weight_decay = self._weight_decay if weight_decay is None else weight_decay
        _check_hyper(lr, betas, eps, weight_decay)
        for flag, on in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable)):
            if on:
                raise NotImplementedError(f"{type(self).__name__}: {flag}=True is not provided")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                      foreach=None, capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=self._kind == "adamw"))


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW, as FusedAdam is torch.optim.Adam (weight_decay defaults to 1e-2 and is decoupled)."""
    _kind = "adamw"
    _cpu_class = torch.optim.AdamW
    _weight_decay = 1e-2


class FusedLamb(_Fused):
    """`Lamb` (vq_ae.optim.lamb.Lamb) in three fused launches per step on device parameters; the trust ratios are formed on
    the device, so no step reads a norm back.  Constructor, defaults and ValueErrors are Lamb's."""
    _kind = "lamb"
    _cpu_class = Lamb

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        for i in (0, 1):
            if not 0.0 <= betas[i] < 1.0:
                raise ValueError(f"Invalid beta parameter at index {i}: {betas[i]}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))


_MIRRORED = {"vq_ae.optim.lamb.Lamb": Lamb}


def _resolve(path):
    if path in _MIRRORED:
        return _MIRRORED[path]
    mod, _, attr = path.rpartition(".")
    return getattr(importlib.import_module(mod), attr)


class SAM(Optimizer):
    """vq_ae.optim.sam.SAM around a base optimiser that shares its param_groups: first_step climbs to w + e(w) along the
    gradient (scaled by w^2 with adaptive=True), second_step goes back to w and lets the base optimiser step with the
    gradients found at the climbed point."""

    def __init__(self, params, base_optimizer_conf, rho=0.05, adaptive=False, **base_optimizer_overrides):
        if not rho >= 0.0:
            raise ValueError(f"Invalid rho, should be non-negative: {rho}")
        super().__init__(params, dict(rho=rho, adaptive=adaptive))
        base = base_optimizer_conf
        if isinstance(base, dict) or hasattr(base, "keys"):
            conf = {k: base[k] for k in base.keys() if k != "params"}
            conf.update(base_optimizer_overrides)
            target = conf.pop("_target_")
            for k in ("_recursive_", "_convert_", "_partial_"):
                conf.pop(k, None)
            if "betas" in conf:
                conf["betas"] = tuple(conf["betas"])
            self.base_optimizer = (_resolve(target) if isinstance(target, str) else target)(self.param_groups, **conf)
        else:
            self.base_optimizer = base(self.param_groups, **base_optimizer_overrides)
        self.param_groups = self.base_optimizer.param_groups

    def _fused(self):
        """The base optimiser where it is a fused one on device tensors: climb and step run in its vqae_optim handle."""
        base = self.base_optimizer
        return base if isinstance(base, _Fused) and base._on_device() else None

    @torch.no_grad()
    def first_step(self, zero_grad=False):
        fused = self._fused()
        if fused is not None:                                      # vqae_optim_sam_first: norm, old_p and climb on the device
            fused._run(True)
            if zero_grad:
                self.zero_grad()
            return
        norm = self._grad_norm()
        for group in self.param_groups:
            scale = group["rho"] / (norm + 1e-12)
            for p in group["params"]:
                if p.grad is None:
                    continue
                self.state[p]["old_p"] = p.data.clone()
                p.add_((torch.pow(p, 2) if group["adaptive"] else 1.0) * p.grad * scale.to(p))
        if zero_grad:
            self.zero_grad()

    @torch.no_grad()
    def second_step(self, zero_grad=False):
        fused = self._fused()
        if fused is not None:                                      # vqae_optim_step reads the saved weights: restore + step
            fused.step()
            if zero_grad:
                self.zero_grad()
            return
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                p.data = self.state[p]["old_p"]
        self.base_optimizer.step()
        if zero_grad:
            self.zero_grad()

    @torch.no_grad()
    def step(self, closure=None):
        if closure is None:
            raise AssertionError("Sharpness Aware Minimization requires closure, but it was not provided")
        closure = torch.enable_grad()(closure)
        self.first_step(zero_grad=True)
        closure()
        self.second_step()

    def _grad_norm(self):
        dev = self.param_groups[0]["params"][0].device
        return torch.norm(torch.stack([((torch.abs(p) if group["adaptive"] else 1.0) * p.grad).norm(p=2).to(dev)
                                       for group in self.param_groups for p in group["params"] if p.grad is not None]), p=2)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self.base_optimizer.param_groups = self.param_groups


_DEFAULTS = {"adam": dict(eps=1e-8, weight_decay=0.0), "adamw": dict(eps=1e-8, weight_decay=0.01),
             "lamb": dict(eps=1e-6, weight_decay=0.0)}


def _base_factory(kind):
    return {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "lamb": Lamb}[kind]


class ClassifierTrainer:
    """ClassifierTrainer(clf, optimizer='adamw' | 'adam' | 'lamb', lr=, betas=, eps=, weight_decay=, sam_rho=None,
    sam_adaptive=False, device=None, loss='bce', class_weight=None, label_smoothing=0.0): trains a private copy of `clf`'s
    weights; `clf` itself changes only in sync_to_module().  loss='bce' (n_out == 1) is Camelyon16BCELoss; loss='ce'
    (n_out = 2 .. 4) is nn.CrossEntropyLoss(weight=class_weight, label_smoothing), the masks being class indices.  eps and
    weight_decay default to the optimiser's own (torch.optim.Adam / AdamW, lamb.py).  The first step decides where it runs
    unless device= says so: tensors in HBM take the HIP path, CPU tensors the torch one."""

    def __init__(self, clf, optimizer="adamw", lr=1e-3, betas=(0.9, 0.999), eps=None, weight_decay=None, sam_rho=None,
                 sam_adaptive=False, device=None, loss="bce", class_weight=None, label_smoothing=0.0):
        if optimizer not in L.OPTIM_KINDS:
            raise ValueError(f"optimizer must be one of {sorted(L.OPTIM_KINDS)}, got {optimizer!r}")
        if loss not in ("bce", "ce"):
            raise ValueError(f"loss must be 'bce' or 'ce', got {loss!r}")
        self.loss = loss
        if loss == "ce":                            # nn.CrossEntropyLoss(weight, label_smoothing) for n_out = 2 .. 4
            self.class_weight, self.label_smoothing = ce_arguments(clf.n_out, class_weight, label_smoothing)
        elif clf.n_out != 1:
            raise ValueError(f"the loss is defined for n_out == 1, this classifier has {clf.n_out}")
        self.clf, self.kind = clf, optimizer
        d = _DEFAULTS[optimizer]
        self.hyper = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(d["eps"] if eps is None else eps),
                          weight_decay=float(d["weight_decay"] if weight_decay is None else weight_decay))
        self.sam_rho = None if sam_rho is None else float(sam_rho)
        self.sam_adaptive = bool(sam_adaptive)
        _base_factory(optimizer)([torch.zeros(1, requires_grad=True)], **self.hyper)          # the optimiser's own ValueErrors
        if self.sam_rho is not None and not self.sam_rho >= 0.0:
            raise ValueError(f"Invalid rho, should be non-negative: {sam_rho}")
        self.device = None
        self._pending = None                       # a state_dict loaded before the first step
        self._native = self._opt_h = None          # HIP path
        self._model = self._opt = None             # torch path
        if device is not None:
            self._ensure(torch.device(device).type)

    # ---- backends ---------------------------------------------------------------------------------
    def _config(self):
        h = self.hyper
        return L.ClassifierOptimConfig(L.OPTIM_KINDS[self.kind], h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"],
                                       -1.0 if self.sam_rho is None else self.sam_rho, int(self.sam_adaptive))

    def _ensure(self, kind):
        if self.device is not None:
            if self.device != kind:
                raise ValueError(f"this trainer runs on {self.device} tensors, got {kind}")
            return
        if kind == "cuda":
            ls = self.clf.layers
            dims = (ls.embedding.num_embeddings, ls.embedding.embedding_dim, ls.in_conv.out_channels, ls.out_conv.out_channels)
            self._native = NativeClassifier(*dims, {"layers." + n: p for n, p in ls.named_parameters()})
            h = ctypes.c_void_p()
            cfg = self._config()
            create = L.lib().vqae_classifier_optim_create_ce if self.loss == "ce" else L.lib().vqae_classifier_optim_create
            L.check(create(self._native._h, ctypes.byref(cfg), ctypes.byref(h)))
            self._opt_h = h
            self._shapes = [tuple(p.shape) for p in _params(self.clf)]
        elif kind == "cpu":
            self._model = copy.deepcopy(self.clf).to(device="cpu", dtype=torch.float32)
            ps = _params(self._model)
            if self.sam_rho is None:
                self._opt = _base_factory(self.kind)(ps, **self.hyper)
            else:
                self._opt = SAM(ps, _base_factory(self.kind), rho=self.sam_rho, adaptive=self.sam_adaptive, **self.hyper)
        else:
            raise ValueError(f"ClassifierTrainer runs on cuda or cpu tensors, got {kind}")
        self.device = kind
        if self._pending is not None:
            sd, self._pending = self._pending, None
            self.load_state_dict(sd)

    def close(self):
        if self._opt_h is not None:
            L.lib().vqae_classifier_optim_destroy(self._opt_h)
            self._opt_h = None
        if self._native is not None:
            self._native.close()
            self._native = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def native(self):
        """The trainer's own NativeClassifier (HIP path): forward on it sees the stepped weights."""
        return self._native

    # ---- the step ----------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, codes, mask, *, pos_weight=1.0, reduction="sum", target=None, target2=None, check=False):
        """One optimiser step on a batch, as loss_and_grads takes it -> (loss float64 [1], stats float64 [B, 6] in
        _lib.CLS_STATS_NAMES order), tensors on the batch's device; nothing is read back.  With SAM both come from the first
        pass (sam.py:62-84 returns those), and target2 is the second pass's soft target (default: target again; the
        reference's loss draws new smoothing noise on its second call).  On CPU tensors stats is one pooled row.
        check=True runs loss_and_grads' validation of labels, targets and codes first: blocking reads."""
        if reduction not in ("sum", "mean"):
            raise ValueError(f"reduction must be 'sum' or 'mean', got {reduction!r}")
        if self.loss == "ce":
            if target is not None or target2 is not None:
                raise ValueError("soft targets belong to the BCE loss; loss='ce' smooths with its label_smoothing")
            return self._step_ce(codes, mask, reduction, check)
        pos_weight = float(pos_weight)
        if not (np.isfinite(pos_weight) and pos_weight >= 0):
            raise ValueError(f"pos_weight must be finite and >= 0, got {pos_weight}")
        codes = _as_codes(codes)
        self._ensure(codes.device.type)
        if mask.dim() == 4 and mask.shape[1] == 1:
            mask = mask[:, 0]
        elif mask.dim() == 2:
            mask = mask[None]
        if tuple(mask.shape) != tuple(codes.shape):
            raise ValueError(f"mask {tuple(mask.shape)} does not match the codes {tuple(codes.shape)}")
        if mask.dtype.is_floating_point:
            raise TypeError(f"the mask holds integer labels, got {mask.dtype}")
        if check and mask.numel() and (int(mask.min()) < 0 or int(mask.max()) > 2):
            raise ValueError("Camelyon16 labels are 0 (background), 1 (tissue) and 2 (cancer)")
        mask = mask.to(device=codes.device, dtype=torch.uint8)
        tgts = []
        for t in (target, target2):
            if t is not None:
                if t.dim() == 2:
                    t = t[None]
                if tuple(t.shape) != tuple(codes.shape):
                    raise ValueError(f"target {tuple(t.shape)} does not match the codes {tuple(codes.shape)}")
                t = t.to(device=codes.device, dtype=torch.float32)
                if check:
                    tv = t[mask != 0]
                    if tv.numel() and (float(tv.min()) < 0 or float(tv.max()) > 1):
                        raise ValueError("soft targets lie in [0, 1]")
            tgts.append(t)
        target, target2 = tgts[0], tgts[1] if tgts[1] is not None else tgts[0]
        if check:
            _check_codes(codes, self.clf.num_embeddings)
            if reduction == "mean" and not bool((mask != 0).any()):
                raise ValueError("reduction='mean' over a batch without a valid code")
        kw = dict(pos_weight=pos_weight, reduction=reduction)
        if self.device == "cuda":
            lib, st = L.lib(), ops._stream()
            loss, g, stats = self._native.loss_grad(codes, mask, target=target, **kw)
            if self.sam_rho is not None:
                L.check(lib.vqae_classifier_optim_sam_first(self._opt_h, ops._p(g), st))
                _, g, _ = self._native.loss_grad(codes, mask, target=target2, **kw)
            L.check(lib.vqae_classifier_optim_step(self._opt_h, ops._p(g), st))
            return loss, stats
        loss, stats = self._cpu_pass(codes, mask, target, pos_weight, reduction)
        if self.sam_rho is not None:
            self._opt.first_step(zero_grad=True)
            self._cpu_pass(codes, mask, target2, pos_weight, reduction)
            self._opt.second_step(zero_grad=True)
        else:
            self._opt.step()
        return loss, stats

    def _step_ce(self, codes, labels, reduction, check):
        """step for loss='ce': `mask` holds the class indices -> (loss float64 [1], stats float64 [B, 20]: the VQAE_CE_* rows;
        one pooled row on CPU tensors), from the first pass with SAM.  check=True: ce_loss_and_grads' validation first.
        Without it nothing is read on the host, as in the BCE step: the labels are cast to uint8 as they are, so they must
        already fit a byte (an int64 label >= 256 would wrap into another class unseen)."""
        codes = _as_codes(codes)
        self._ensure(codes.device.type)
        labels = _as_labels(labels, codes)
        no = self.clf.n_out
        if check:
            if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= no):
                raise ValueError(f"labels are class indices 0 .. {no - 1}")
            _check_codes(codes, self.clf.num_embeddings)
            if reduction == "mean" and not ce_weight_sum(labels, self.class_weight, no) > 0:
                raise ValueError("reduction='mean' over a batch whose class weights sum to zero")
        labels = labels.to(device=codes.device, dtype=torch.uint8)
        kw = dict(weight=self.class_weight, label_smoothing=self.label_smoothing, reduction=reduction)
        if self.device == "cuda":
            lib, st = L.lib(), ops._stream()
            loss, g, stats = self._native.loss_grad_ce(codes, labels, **kw)
            if self.sam_rho is not None:
                L.check(lib.vqae_classifier_optim_sam_first(self._opt_h, ops._p(g), st))
                _, g, _ = self._native.loss_grad_ce(codes, labels, **kw)
            L.check(lib.vqae_classifier_optim_step(self._opt_h, ops._p(g), st))
            return loss, stats
        loss, stats = self._cpu_pass_ce(codes, labels, reduction)
        if self.sam_rho is not None:
            self._opt.first_step(zero_grad=True)
            self._cpu_pass_ce(codes, labels, reduction)
            self._opt.second_step(zero_grad=True)
        else:
            self._opt.step()
        return loss, stats

    def _cpu_pass_ce(self, codes, labels, reduction):
        grads, (conf, wsum, nll, smooth, n_bad), loss = torch_ce_loss_grad(self._model, codes, labels, self.class_weight,
                                                                             self.label_smoothing, reduction)
        for p, g in zip(_params(self._model), grads):
            p.grad = g.detach().clone()
        row = torch.zeros((1, L.CE_STATS_K), dtype=torch.float64)
        no = conf.shape[0]
        for l in range(no):
            for q in range(no):
                row[0, l * 4 + q] = float(conf[l, q])
        row[0, L.CE_WEIGHT_SUM], row[0, L.CE_NLL_SUM], row[0, L.CE_SMOOTH_SUM], row[0, L.CE_N_BAD] = wsum, nll, smooth, n_bad
        return torch.tensor([loss], dtype=torch.float64), row

    def _cpu_pass(self, codes, mask, target, pos_weight, reduction):
        grads, (tp, fp, fn, tn, loss_sum) = torch_loss_grad(self._model, codes, mask, target, pos_weight, reduction)
        for p, g in zip(_params(self._model), grads):
            p.grad = g.detach().clone()
        n = tp + fp + fn + tn
        loss = loss_sum / n if reduction == "mean" else loss_sum
        return (torch.tensor([loss], dtype=torch.float64),
                torch.tensor([[tp, fp, fn, tn, n, loss_sum]], dtype=torch.float64))

    # ---- hyper-parameters, weights, state ------------------------------------------------------------
    def set_lr(self, lr):
        """The learning rate of the following steps (an lr schedule's assignment to param_groups[0]['lr'])."""
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        self.hyper["lr"] = float(lr)
        self._push_hyper()

    def _push_hyper(self):
        if self.device == "cuda":
            cfg = self._config()
            L.check(L.lib().vqae_classifier_optim_set(self._opt_h, ctypes.byref(cfg)))
        elif self.device == "cpu":
            for g in self._opt.param_groups:
                g.update(lr=self.hyper["lr"], betas=self.hyper["betas"], eps=self.hyper["eps"],
                         weight_decay=self.hyper["weight_decay"])

    def weights(self):
        """The current weights: seven fp32 CPU tensors in PARAM_NAMES order (one blocking download on the HIP path)."""
        if self.device == "cuda":
            outs = [np.empty(s, np.float32) for s in self._shapes]
            arr = (ctypes.c_void_p * 7)(*[o.ctypes.data for o in outs])
            L.check(L.lib().vqae_classifier_download(self._native._h, arr, ops._stream()))
            return [torch.from_numpy(o) for o in outs]
        src = self._model if self.device == "cpu" else self.clf
        return [p.detach().to(device="cpu", dtype=torch.float32).clone() for p in _params(src)]

    @torch.no_grad()
    def sync_to_module(self):
        """Copies the trained weights into `clf`'s parameters in place (their device and dtype); -> clf."""
        for p, w in zip(_params(self.clf), self.weights()):
            p.copy_(w)
        return self.clf

    def _group(self):
        g = dict(self.hyper)
        if self.kind != "lamb":
            g.update(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                     decoupled_weight_decay=self.kind == "adamw")
        if self.sam_rho is not None:
            g.update(rho=self.sam_rho, adaptive=self.sam_adaptive)
        g["params"] = list(range(7))
        return g

    def state_dict(self):
        """torch.optim's layout: {'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [{...}]} over the seven
        parameters in PARAM_NAMES order; what torch.optim.Adam / AdamW / Lamb.load_state_dict take (step is a float32 scalar
        tensor for Adam / AdamW, as torch keeps it, and an int for Lamb).  State tensors are on the CPU."""
        if self.device == "cpu":
            base = self._opt.base_optimizer if self.sam_rho is not None else self._opt
            return base.state_dict()
        if self.device is None:
            return copy.deepcopy(self._pending) if self._pending is not None else {"state": {}, "param_groups": [self._group()]}
        n = sum(int(np.prod(s)) for s in self._shapes)
        m, v, step = np.empty(n, np.float32), np.empty(n, np.float32), ctypes.c_int64()
        L.check(L.lib().vqae_classifier_optim_export(self._opt_h, m.ctypes.data, v.ctypes.data, ctypes.byref(step), ops._stream()))
        state, o = {}, 0
        if step.value:
            for i, s in enumerate(self._shapes):
                k = int(np.prod(s))
                state[i] = {"step": step.value if self.kind == "lamb" else torch.tensor(float(step.value), dtype=torch.float32),
                            "exp_avg": torch.from_numpy(m[o:o + k].reshape(s).copy()),
                            "exp_avg_sq": torch.from_numpy(v[o:o + k].reshape(s).copy())}
                o += k
        return {"state": state, "param_groups": [self._group()]}

    def load_state_dict(self, sd):
        """Takes a state_dict of this class or of torch.optim.Adam / AdamW / Lamb over the seven parameters: the moments, the
        step count (one for all seven) and lr, betas, eps, weight_decay of its single param group."""
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != 7:
            raise ValueError("ClassifierTrainer.load_state_dict: one param group over the seven parameters expected")
        ids = list(groups[0]["params"])
        state = sd["state"]
        if len(state) not in (0, 7):
            raise ValueError(f"ClassifierTrainer.load_state_dict: state for {len(state)} of 7 parameters")
        steps = {int(state[i]["step"]) for i in ids} if state else {0}
        if len(steps) != 1:
            raise ValueError(f"ClassifierTrainer.load_state_dict: the parameters are at different steps {sorted(steps)}")
        g = groups[0]
        self.hyper = dict(lr=float(g["lr"]), betas=(float(g["betas"][0]), float(g["betas"][1])), eps=float(g["eps"]),
                          weight_decay=float(g["weight_decay"]))
        if self.device is None:
            self._pending = copy.deepcopy(sd)
            return
        if self.device == "cpu":
            base = self._opt.base_optimizer if self.sam_rho is not None else self._opt
            own = base.state_dict()["param_groups"][0]
            merged = dict(own)
            merged.update({k: g[k] for k in ("lr", "betas", "eps", "weight_decay")})
            st = {j: {k: (v if k != "step" or self.kind == "lamb" else torch.as_tensor(float(v), dtype=torch.float32))
                      for k, v in state[i].items() if k in ("step", "exp_avg", "exp_avg_sq")} for j, i in enumerate(ids)} if state else {}
            if self.kind == "lamb":
                for s in st.values():
                    s["step"] = int(s["step"])
            base.load_state_dict({"state": st, "param_groups": [merged]})
            if self.sam_rho is not None:
                self._opt.param_groups = base.param_groups
            return
        self._push_hyper()
        shapes = self._shapes
        n = sum(int(np.prod(s)) for s in shapes)
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        if state:
            o = 0
            for i, s in zip(ids, shapes):
                k = int(np.prod(s))
                for dst, key in ((m, "exp_avg"), (v, "exp_avg_sq")):
                    t = state[i][key]
                    if tuple(t.shape) != s:
                        raise ValueError(f"ClassifierTrainer.load_state_dict: {key} of parameter {i} has shape {tuple(t.shape)}, not {s}")
                    dst[o:o + k] = t.detach().to(device="cpu", dtype=torch.float32).reshape(-1).numpy()
                o += k
        L.check(L.lib().vqae_classifier_optim_import(self._opt_h, m.ctypes.data, v.ctypes.data, steps.pop(), ops._stream()))


__all__ = ["Lamb", "SAM", "FusedAdam", "FusedAdamW", "FusedLamb", "ClassifierTrainer", "PARAM_NAMES"]
