"""The downstream consumer of the stored code grids: the reference's `validation_nn` CNNClassifier.

`save_encodings_hdf5` leaves one code grid per slide under `images/<stem>` and, with labels, `masks/<stem>_mask`; the
reference trains a small CNN on exactly that file (validation_nn/model.py, conf/model/cnn_classifier.yaml):

    nn.Embedding(256, 1) -> FlattenAfterEmbedding -> Conv2d(1, 8, 3, pad 1, bias) -> ELU -> Conv2d(8, 8, 3) -> ELU
    -> Conv2d(8, 1, 3)

a per-code tumour logit for a whole slide.  `CNNClassifier` mirrors that module for inference (training is functional, in
classifier_train.py: `loss_and_grads` writes `.grad` from the fused backward and any torch.optim optimiser steps): on tensors in HBM its forward
is one fused HIP launch (csrc/classifier.hip); on CPU tensors it is a plain torch restatement of the same layers, the
yardstick the tests pin against the reference's recorded output.  `classify_slide` / `classify_hdf5` add what the codes
were made for: the uint8 probability map at code resolution and the masked precision / recall / BCE of
`Camelyon16BCELoss` (utils/train_helpers.py:101-138), from the same launch.

State-dict names.  The reference's `SequentialFromKwargs` (validation_nn/layers/misc.py:4-6) hands `kwargs.values()` to
nn.Sequential, so its keyword names are dropped and a reference checkpoint says `layers.0.weight`, `layers.2.weight`,
`layers.2.bias`, ... .  The mirror keeps cnn_classifier.yaml's names for its children (`layers.embedding`,
`layers.in_conv`, ...; the C ABI takes the tensors under those names) and speaks the reference's positional names in
`state_dict()`; `load_state_dict()` takes either spelling.
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from . import hdf5
from . import ops

LAYER_NAMES = ("embedding", "flatten_after_embedding", "in_conv", "act1", "hidden_conv1", "act2", "out_conv")
_POSITION = {name: str(i) for i, name in enumerate(LAYER_NAMES)}
_NAME_AT = {v: k for k, v in _POSITION.items()}


class FlattenAfterEmbedding(nn.Module):
    """[B, C, *dims, E] -> [B, C * E, *dims] (validation_nn/layers/misc.py:9-22): the embedding vector becomes channels."""

    def forward(self, batch):
        return batch.movedim(-1, 2).flatten(1, 2)


class NativeClassifier:
    """Owns a vqae_classifier built from {name: tensor} under cnn_classifier.yaml's layer names (`layers.in_conv.weight`...)."""

    def __init__(self, num_embeddings, embedding_dim, hidden, n_out, tensors):
        self.num_embeddings, self.n_out = int(num_embeddings), int(n_out)
        self.dims = (int(num_embeddings), int(embedding_dim), int(hidden), int(n_out))
        keep, arr = self._tensor_array(tensors)
        h = ctypes.c_void_p()
        L.check(L.lib().vqae_classifier_create(*self.dims, arr, len(arr), ctypes.byref(h)))
        self._h = h

    @staticmethod
    def _tensor_array(tensors):
        keep, items = [], []
        for name, t in tensors.items():
            a = np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t), dtype=np.float32)
            keep.append(a)
            items.append(L.Tensor(name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size))
        return keep, (L.Tensor * len(items))(*items)

    def update(self, tensors):
        """New weights of the same shapes into the existing handle (vqae_classifier_update): what an optimiser step needs."""
        keep, arr = self._tensor_array(tensors)
        L.check(L.lib().vqae_classifier_update(self._h, arr, len(arr)))

    def loss_grad(self, codes, mask, target=None, pos_weight=1.0, reduction="sum"):
        """codes, mask [B,H,W] in HBM -> (loss [1], packed grads, stats [B,6]) in fp64, see ops.classifier_loss_grad"""
        return ops.classifier_loss_grad(self._h, codes, mask, target=target, pos_weight=pos_weight, reduction=reduction)

    def forward(self, codes, logits=True, heat=False, mask=None, pos_weight=1.0):
        """codes [B,H,W] in HBM -> (logits | None, heat | None, stats | None), see ops.classifier_forward"""
        return ops.classifier_forward(self._h, codes, self.n_out, logits=logits, heat=heat, mask=mask, pos_weight=pos_weight)

    def forward_ce(self, codes, logits=False, prob=False, cls=True, labels=None, weight=None, label_smoothing=0.0):
        """codes [B,H,W] in HBM -> (logits | None, prob | None, class | None, stats [B,20] | None), see ops.classifier_forward_ce"""
        return ops.classifier_forward_ce(self._h, codes, self.n_out, logits=logits, prob=prob, cls=cls, labels=labels,
                                         weight=weight, label_smoothing=label_smoothing)

    def loss_grad_ce(self, codes, labels, weight=None, label_smoothing=0.0, reduction="mean"):
        """codes, labels [B,H,W] in HBM -> (loss [1], packed grads, stats [B,20]) in fp64, see ops.classifier_loss_grad_ce"""
        return ops.classifier_loss_grad_ce(self._h, codes, labels, self.n_out, weight=weight, label_smoothing=label_smoothing,
                                           reduction=reduction)

    def close(self):
        if getattr(self, "_h", None):
            L.lib().vqae_classifier_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _as_codes(data):
    """integer codes [B,1,H,W] / [B,H,W] / [H,W] -> [B,H,W] (a view)"""
    if data.dtype.is_floating_point or data.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise TypeError(f"CNNClassifier takes integer codes, got {data.dtype}")
    if data.dim() == 4:
        if data.shape[1] != 1:
            raise ValueError(f"codes [B,1,H,W] expected, got {tuple(data.shape)}")
        return data[:, 0]
    if data.dim() == 3:
        return data
    if data.dim() == 2:
        return data[None]
    raise ValueError(f"codes must be [B,1,H,W], [B,H,W] or [H,W]; got {tuple(data.shape)}")


def _check_codes(codes, num_embeddings):
    """IndexError for a code outside 0 .. K-1, as nn.Embedding raises it: one min / max on the tensor's own device, skipped
    where the dtype cannot leave the table."""
    if codes.numel() == 0 or (codes.dtype == torch.uint8 and num_embeddings >= 256):
        return
    c = codes.to(torch.int32) if codes.dtype == getattr(torch, "uint16", None) else codes
    lo, hi = int(c.min()), int(c.max())
    if lo < 0 or hi >= num_embeddings:
        raise IndexError(f"index out of range in self: codes span {lo} .. {hi}, the embedding has {num_embeddings} rows")


def _conv3x3(x, w, b):
    """3x3 / stride 1 / zero-pad 1 convolution of the restatement.  For fp32 on the CPU it names ATen's oneDNN convolution
    instead of leaving the choice to F.conv2d: that dispatcher sends a batch, or a large image, to oneDNN's direct kernels but
    a single small image (at most 20480 elements) to an im2col + BLAS GEMM, whose sums differ between machines and thread
    counts (1.7e-6 on a 7 x 5 grid was seen), so a slide alone and the same slide in a batch would differ by as much.  On the
    oneDNN route they agree to an ulp (2.4e-7 at most on the fixture grids), at any thread count."""
    if x.device.type == "cpu" and x.dtype == torch.float32 and torch.backends.mkldnn.is_available() and torch.backends.mkldnn.enabled:
        return torch.mkldnn_convolution(x.contiguous(), w, b, [1, 1], [1, 1], [1, 1], 1)
    return F.conv2d(x, w, b, padding=1)


class CNNClassifier(nn.Module):
    """Inference mirror of validation_nn.model.CNNClassifier over the layers of conf/model/cnn_classifier.yaml.

    CNNClassifier(num_embeddings=256, embedding_dim=1, hidden=8, n_out=1) builds the shipped stack; `layers=` takes an
    already built stack of the same seven modules instead (what Hydra hands the reference's constructor), and the
    training-only arguments of the reference (optim, loss_f, lr_scheduler, *_metrics) are accepted and ignored.  Anything
    but Embedding -> flatten -> 3x3 zero-pad biased conv -> ELU(1) -> 3x3 conv -> ELU(1) -> 3x3 conv raises
    NotImplementedError."""

    def __init__(self, num_embeddings=256, embedding_dim=1, hidden=8, n_out=1, *, layers=None, **reference_kwargs):
        super().__init__()
        unknown = set(reference_kwargs) - {"optim", "loss_f", "lr_scheduler", "train_metrics", "val_metrics", "test_metrics"}
        if unknown:
            raise TypeError(f"CNNClassifier: unexpected arguments {sorted(unknown)}")
        if layers is None:
            mods = [nn.Embedding(num_embeddings, embedding_dim), FlattenAfterEmbedding(),
                    nn.Conv2d(embedding_dim, hidden, 3, padding=1), nn.ELU(),
                    nn.Conv2d(hidden, hidden, 3, padding=1), nn.ELU(),
                    nn.Conv2d(hidden, n_out, 3, padding=1)]
        else:
            mods = list(layers.children())
            if len(mods) != len(LAYER_NAMES):
                raise NotImplementedError(f"CNNClassifier: a stack of {len(mods)} layers; the implemented one is {LAYER_NAMES}")
            if type(mods[1]).__name__ == "FlattenAfterEmbedding":
                mods[1] = FlattenAfterEmbedding()
        self.layers = nn.Sequential(OrderedDict(zip(LAYER_NAMES, mods)))
        self._check_structure()
        self._native = None
        self.training = False
        for m in self.modules():
            m.training = False
        self._register_state_dict_hook(self._reference_names)
        self._register_load_state_dict_pre_hook(self._yaml_names)

    # ---- structure ------------------------------------------------------------------------------
    def _check_structure(self):
        ls = self.layers
        if tuple(n for n, _ in ls.named_children()) != LAYER_NAMES:
            raise NotImplementedError(f"CNNClassifier: layers {[n for n, _ in ls.named_children()]} are not {LAYER_NAMES}")
        emb = ls.embedding
        if type(emb) is not nn.Embedding or emb.padding_idx is not None or emb.max_norm is not None:
            raise NotImplementedError("CNNClassifier: `embedding` must be a plain nn.Embedding (layers/misc/embedding.yaml)")
        if not isinstance(ls.flatten_after_embedding, FlattenAfterEmbedding):
            raise NotImplementedError("CNNClassifier: `flatten_after_embedding` must be FlattenAfterEmbedding")
        cin = emb.embedding_dim
        for name in ("in_conv", "hidden_conv1", "out_conv"):
            c = getattr(ls, name)
            if (type(c) is not nn.Conv2d or c.kernel_size != (3, 3) or c.stride != (1, 1) or c.padding != (1, 1)
                    or c.dilation != (1, 1) or c.groups != 1 or c.padding_mode != "zeros" or c.bias is None):
                raise NotImplementedError(f"CNNClassifier: `{name}` must be Conv2d(k3, s1, p1, zeros, bias) (same2d.yaml); got {c}")
            if c.in_channels != cin:
                raise NotImplementedError(f"CNNClassifier: `{name}` takes {c.in_channels} channels, its input has {cin}")
            cin = c.out_channels
        if ls.in_conv.out_channels != ls.hidden_conv1.out_channels:
            raise NotImplementedError("CNNClassifier: one hidden width is implemented (in_conv and hidden_conv1 differ)")
        for name in ("act1", "act2"):
            a = getattr(ls, name)
            if type(a) is not nn.ELU or a.alpha != 1.0:
                raise NotImplementedError(f"CNNClassifier: `{name}` must be ELU(alpha=1) (activation/elu.yaml); got {a}")

    @property
    def num_embeddings(self):
        return self.layers.embedding.num_embeddings

    @property
    def n_out(self):
        return self.layers.out_conv.out_channels

    # ---- state-dict naming ------------------------------------------------------------------------
    @staticmethod
    def _reference_names(module, state_dict, prefix, local_metadata):
        for k in [k for k in state_dict if k.startswith(prefix + "layers.")]:
            name, _, rest = k[len(prefix) + 7:].partition(".")
            if name in _POSITION:
                state_dict[f"{prefix}layers.{_POSITION[name]}.{rest}"] = state_dict.pop(k)
        return state_dict

    @staticmethod
    def _yaml_names(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for k in [k for k in state_dict if k.startswith(prefix + "layers.")]:
            pos, _, rest = k[len(prefix) + 7:].partition(".")
            if pos in _NAME_AT:
                state_dict[f"{prefix}layers.{_NAME_AT[pos]}.{rest}"] = state_dict.pop(k)

    def load_state_dict(self, state_dict, *a, **k):
        r = super().load_state_dict(OrderedDict(state_dict), *a, **k)      # (a copy: the renaming hook edits its argument)
        self.refresh()
        return r

    # ---- inference only ---------------------------------------------------------------------------
    def train(self, mode=True):
        if mode:
            raise NotImplementedError("vqae_amd.classifier.CNNClassifier is inference-only (the HIP path has no autograd)")
        return super().train(False)

    def refresh(self):
        """Drop the device snapshot of the weights (call after changing parameters)."""
        if self._native is not None:
            self._native[1].close()
        self._native = None

    def native(self):
        """The vqae_classifier of the current weights: built on first use; when a parameter changed or was replaced (an
        optimiser step) the same handle takes the new weights, and only another shape builds a new one."""
        self._check_structure()
        sig = tuple((id(t), t._version) for t in self.parameters())
        if self._native is None or self._native[0] != sig:
            ls = self.layers
            tensors = {"layers." + n: p for n, p in ls.named_parameters()}
            dims = (ls.embedding.num_embeddings, ls.embedding.embedding_dim, ls.in_conv.out_channels, ls.out_conv.out_channels)
            if self._native is not None and self._native[1].dims == dims:
                self._native[1].update(tensors)
                self._native = (sig, self._native[1])
            else:
                self.refresh()
                self._native = (sig, NativeClassifier(*dims, tensors))
        return self._native[1]

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_native"] = None
        return d

    def reference_forward(self, codes):
        """The same layers in plain torch on whatever device the codes are on: embedding -> permute -> conv2d(padding=1) -> elu
        -> conv2d -> elu -> conv2d.  codes [B,H,W] -> [B,n_out,H,W] fp32 (or the parameters' dtype)."""
        ls = self.layers
        idx = codes if codes.dtype in (torch.int32, torch.int64) else codes.to(torch.int64)
        x = F.embedding(idx.long()[:, None], ls.embedding.weight)        # [B,1,H,W,E]
        x = ls.flatten_after_embedding(x).contiguous()                   # [B,E,H,W]: the vector becomes channels
        x = F.elu(_conv3x3(x, ls.in_conv.weight, ls.in_conv.bias))
        x = F.elu(_conv3x3(x, ls.hidden_conv1.weight, ls.hidden_conv1.bias))
        return _conv3x3(x, ls.out_conv.weight, ls.out_conv.bias)

    def forward(self, data):
        if torch.is_grad_enabled() and data.requires_grad:
            raise NotImplementedError("vqae_amd.classifier.CNNClassifier is inference-only: inputs that require grad are not supported")
        codes = _as_codes(data)
        _check_codes(codes, self.num_embeddings)
        with torch.no_grad():
            if codes.is_cuda:
                return self.native().forward(codes)[0]
            return self.reference_forward(codes)


# ---- scoring ----------------------------------------------------------------------------------------
def _summary(tp, fp, fn, tn, loss_sum):
    n = tp + fp + fn + tn
    nan = float("nan")
    return {"tp": int(tp), "fp": int(fp), "fn": int(fn), "tn": int(tn), "n_valid": int(n),
            "loss_sum": float(loss_sum), "loss": float(loss_sum) / n if n else nan,
            "precision": tp / (tp + fp) if tp + fp else nan, "recall": tp / (tp + fn) if tp + fn else nan}


def _score_host(logit, mask, pos_weight):
    """(heat uint8 [H,W], counts + loss sum) from one slide's logits [H,W] with torch on the host, in fp64: the scoring of
    the path with an injected forward"""
    x = logit.double()
    heat = torch.round(255.0 * torch.sigmoid(x)).to(torch.uint8)
    if mask is None:
        return heat, None
    valid = mask != 0
    t = (mask >= 2)[valid]
    xv = x[valid]
    pr = xv > 0
    loss = (pos_weight * F.softplus(-xv[t])).sum() + F.softplus(xv[~t]).sum()
    return heat, (int((pr & t).sum()), int((pr & ~t).sum()), int((~pr & t).sum()), int((~pr & ~t).sum()), float(loss))


# ---- multi-class scoring: nn.CrossEntropyLoss and the confusion matrix ---------------------------------------------------
def ce_arguments(n_out, class_weight, label_smoothing):
    """(class_weight as a list of n_out floats or None, label_smoothing as a float), checked as nn.CrossEntropyLoss and the
    library check them.  ValueError: n_out == 1, a weight vector of another length, a negative or non-finite weight,
    label_smoothing outside [0, 1]."""
    if not 2 <= n_out <= 4:
        raise ValueError(f"the cross-entropy loss is defined for n_out = 2 .. 4, this classifier has {n_out}")
    w = None
    if class_weight is not None:
        w = [float(v) for v in (class_weight.tolist() if hasattr(class_weight, "tolist") else class_weight)]
        if len(w) != n_out:
            raise ValueError(f"class_weight has {len(w)} entries, the classifier {n_out} outputs")
        if not all(np.isfinite(v) and v >= 0 for v in w):
            raise ValueError(f"class weights must be finite and >= 0, got {w}")
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1], got {label_smoothing}")
    return w, eps


def apply_background_hack(confusion):
    """`out[:, 0][labels == 0] = inf` (validation_nn/model.py:103) on raw counts [label, prediction]: every position labelled
    0 is predicted 0, so row 0 collapses into column 0.  -> a new int64 array"""
    c = np.array(confusion, dtype=np.int64)
    c[0, 0] = c[0].sum()
    c[0, 1:] = 0
    return c


def ce_summary(confusion, weight_sum, nll_sum, smooth_sum, n_bad, label_smoothing, hack=True):
    """Scores from raw counts [n_out, n_out] at [label, prediction] and the loss sums of a VQAE_CE_* stats row (or of several
    rows added up): 'confusion' (after apply_background_hack when hack), per-class 'precision' = diag / column sum and 'recall' =
    diag / row sum (nan on an empty denominator), 'loss_sum' = (1 - eps) * nll + (eps / n_out) * smooth, 'weight_sum',
    'loss' = loss_sum / weight_sum (nan for a zero weight sum) and 'n_bad' (labels >= n_out, counted nowhere else)."""
    c = apply_background_hack(confusion) if hack else np.array(confusion, dtype=np.int64)
    no = c.shape[0]
    nan = float("nan")
    col, row = c.sum(0), c.sum(1)
    loss_sum = (1.0 - label_smoothing) * float(nll_sum) + (label_smoothing / no) * float(smooth_sum)
    return {"confusion": c, "precision": [int(c[k, k]) / int(col[k]) if col[k] else nan for k in range(no)],
            "recall": [int(c[k, k]) / int(row[k]) if row[k] else nan for k in range(no)],
            "loss_sum": loss_sum, "weight_sum": float(weight_sum), "loss": loss_sum / float(weight_sum) if weight_sum else nan,
            "n_bad": int(n_bad)}


def ce_pooled(confusion, weight_sum, loss_sum, n_bad):
    """ce_summary's dict for scores that are already summaries -- counts after the hack, loss sums already mixed -- added up
    over slides or steps: loss = summed loss / summed weight."""
    return ce_summary(confusion, weight_sum, loss_sum, 0.0, n_bad, 0.0, hack=False)


def ce_stats_rows(stats, n_out):
    """VQAE_CE_* rows (tensor or array [B, 20]) summed over the batch -> (confusion [n_out, n_out], weight_sum, nll_sum,
    smooth_sum, n_bad)"""
    r = np.asarray(stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.float64).reshape(-1, L.CE_STATS_K)
    conf = np.rint(r[:, :16]).astype(np.int64).sum(0).reshape(4, 4)[:n_out, :n_out]
    return conf, float(r[:, L.CE_WEIGHT_SUM].sum()), float(r[:, L.CE_NLL_SUM].sum()), float(r[:, L.CE_SMOOTH_SUM].sum()), \
        int(np.rint(r[:, L.CE_N_BAD]).sum())


def ce_stats_host(logits, labels, weight, n_out):
    """The same five numbers from logits [B,n_out,H,W] and labels [B,H,W] with torch, in fp64, on the tensors' device."""
    x = logits.double()
    lp = F.log_softmax(x, dim=1)
    pred = x.argmax(dim=1)
    lab = labels.long()
    ok = lab < n_out
    w = torch.ones(n_out, dtype=torch.float64, device=x.device) if weight is None else \
        torch.as_tensor(weight, dtype=torch.float64, device=x.device)
    conf = torch.bincount(lab[ok] * n_out + pred[ok], minlength=n_out * n_out).reshape(n_out, n_out).cpu().numpy().astype(np.int64)
    lpo = lp.movedim(1, -1)[ok]                                    # [n, n_out]
    y = lab[ok]
    wy = w[y]
    nll = -(wy * lpo.gather(1, y[:, None])[:, 0]).sum()
    smooth = -(lpo * w).sum()
    return conf, float(wy.sum()), float(nll), float(smooth), int((~ok).sum())


def _classify_slide_ce(clf, g, m, logits, prob, class_weight, label_smoothing, hack, forward_fn):
    no = clf.n_out
    w, eps = ce_arguments(no, class_weight, label_smoothing)
    if m is not None and m.numel() and int(m.max()) >= no:
        raise ValueError(f"labels are class indices 0 .. {no - 1}, got {int(m.max())}")
    out = {}
    if forward_fn is not None:
        _check_codes(g, clf.num_embeddings)
        lg = forward_fn(g[None, None])
        if tuple(lg.shape) != (1, no) + tuple(g.shape):
            raise ValueError(f"forward_fn returned {tuple(lg.shape)}")
        lg = lg.cpu()
        if logits:
            out["logits"] = lg[0].float().numpy()
        out["class"] = lg[0].double().argmax(0).to(torch.uint8).numpy()
        if prob:
            out["prob"] = torch.round(255.0 * torch.softmax(lg[0].double(), 0)).to(torch.uint8).numpy()
        if m is not None:
            out.update(ce_summary(*ce_stats_host(lg, m[None], w, no), eps, hack))
        return out
    g = g.to("cuda")                                               # raises without a GPU: there is no CPU fallback
    _check_codes(g, clf.num_embeddings)
    lg, pr, cl, st = clf.native().forward_ce(g[None], logits=logits, prob=prob, cls=True,
                                             labels=m.to("cuda")[None] if m is not None else None, weight=w, label_smoothing=eps)
    if logits:
        out["logits"] = lg[0].cpu().numpy()
    if prob:
        out["prob"] = pr[0].cpu().numpy()
    out["class"] = cl[0].cpu().numpy()
    if st is not None:
        out.update(ce_summary(*ce_stats_rows(st, no), eps, hack))
    return out


def _grid_tensor(a, what):
    if isinstance(a, torch.Tensor):
        t = a
    else:
        a = np.asarray(a)
        if a.dtype == np.bool_:                                    # cast_to_lowest_dtype stores a {0, 1} grid as bool
            a = a.astype(np.uint8)
        elif a.dtype not in (np.uint8, np.uint16, np.int32, np.int64):
            if a.dtype.kind not in "iu":
                raise TypeError(f"{what} must hold integers, got {a.dtype}")
            a = a.astype(np.int32 if a.dtype.itemsize <= 2 else np.int64)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2:
        raise ValueError(f"{what} must be 2-D, got shape {tuple(t.shape)}")
    return t


@torch.no_grad()
def classify_slide(clf, grid, mask=None, *, heat=True, logits=False, pos_weight=1.0, forward_fn=None, loss="bce",
                   class_weight=None, label_smoothing=0.0, background_hack=True, prob=False):
    """One stored code grid [H,W] (array as stored, or a tensor) -> dict of host arrays and scores:
      'heat'   uint8 [H,W] = rint(255 * sigmoid(logit)), the tumour probability per code (n_out == 1), when heat=True;
      'logits' fp32 [n_out,H,W], when logits=True;
      with `mask` ([H,W]; 0 background, 1 tissue, 2 cancer) also tp, fp, fn, tn, n_valid over the codes with mask != 0
      (target mask - 1, prediction logit > 0), loss_sum = Camelyon16BCELoss(reduction='sum', pos_weight, no smoothing),
      loss = loss_sum / n_valid,
      precision and recall (nan on an empty denominator).
    The grid goes to the GPU once and one fused launch produces everything asked for.  forward_fn(codes [1,1,H,W]) ->
    logits [1,n_out,H,W] replaces the HIP path (CPU tests of the host logic, like run_eval's encode_fn): heat and scores
    are then formed from its logits on the host in fp64.
    loss='ce' (n_out = 2 .. 4) scores with nn.CrossEntropyLoss(weight=class_weight, label_smoothing) instead, the mask
    bytes being the class indices (conf/model/loss_f/cross_entropy.yaml): 'class' uint8 [H,W] = argmax over the classes
    (always), 'prob' uint8 [n_out,H,W] = rint(255 * softmax) with prob=True, 'logits' as above, and with `mask` the scores
    of ce_summary: the n_out x n_out 'confusion' at [label, prediction], per-class 'precision' and 'recall', 'loss_sum',
    'weight_sum', 'loss' (the 'mean' reduction) and 'n_bad'.  background_hack (default on) applies the
    `out[:, 0][labels == 0] = inf` of validation_nn/model.py:103 to the counts; heat and pos_weight are not used.
    IndexError: a code outside the embedding table.  ValueError: shapes that do not match, labels outside 0 .. 2 (loss='ce':
    a label >= n_out), an unknown loss, loss='ce' with n_out == 1."""
    if loss not in ("bce", "ce"):
        raise ValueError(f"loss must be 'bce' or 'ce', got {loss!r}")
    g = _grid_tensor(grid, "code grid")
    m = None
    if mask is not None:
        m = _grid_tensor(mask, "mask")
        if tuple(m.shape) != tuple(g.shape):
            raise ValueError(f"mask {tuple(m.shape)} does not match the code grid {tuple(g.shape)}")
    if loss == "ce":
        if m is not None and m.numel() and (int(m.min()) < 0 or int(m.max()) > 255):
            raise ValueError("labels are class indices stored as bytes")
        return _classify_slide_ce(clf, g, None if m is None else m.to(torch.uint8), logits, prob, class_weight, label_smoothing,
                                  background_hack, forward_fn)
    if m is not None:
        if m.numel() and (int(m.min()) < 0 or int(m.max()) > 2):
            raise ValueError("Camelyon16 labels are 0 (background), 1 (tissue) and 2 (cancer)")
        m = m.to(torch.uint8)
    if (heat or m is not None) and clf.n_out != 1:
        raise ValueError(f"heat and scores are defined for n_out == 1, this classifier has {clf.n_out}")
    if not (heat or logits or m is not None):
        raise ValueError("classify_slide: nothing requested")
    out = {}
    if forward_fn is not None:
        _check_codes(g, clf.num_embeddings)
        lg = forward_fn(g[None, None])
        if tuple(lg.shape) != (1, clf.n_out) + tuple(g.shape):
            raise ValueError(f"forward_fn returned {tuple(lg.shape)}")
        if logits:
            out["logits"] = lg[0].float().cpu().numpy()
        if heat or m is not None:
            h, st = _score_host(lg[0, 0].cpu(), m.cpu() if m is not None else None, float(pos_weight))
            if heat:
                out["heat"] = h.numpy()
            if st is not None:
                out.update(_summary(*st))
        return out
    g = g.to("cuda")                                               # raises without a GPU: there is no CPU fallback
    _check_codes(g, clf.num_embeddings)
    lg, h, st = clf.native().forward(g[None], logits=logits, heat=heat, mask=m.to("cuda")[None] if m is not None else None,
                                     pos_weight=float(pos_weight))
    if logits:
        out["logits"] = lg[0].cpu().numpy()
    if heat:
        out["heat"] = h[0].cpu().numpy()
    if st is not None:
        tp, fp, fn, tn, _, loss_sum = st[0].tolist()
        out.update(_summary(int(tp), int(fp), int(fn), int(tn), loss_sum))
    return out


def classify_hdf5(clf, path, out_path=None, *, names=None, forward_fn=None, pos_weight=1.0, loss="bce", class_weight=None,
                  label_smoothing=0.0, background_hack=True):
    """Every slide of an archive written by save_encodings_hdf5 / convert_npy_to_hdf5: `images/<stem>` with
    `masks/<stem>_mask` where present, in sorted key order (the order of the reference's dataset,
    datamodules/camelyon16.py:226-235).  names: the stems to take (default: all).  out_path: an HDF5 file that receives the
    uint8 probability maps as `predictions/<stem>`.
    -> {'slides': {stem: classify_slide's scores, {} for a slide without a mask}, 'pooled': the scores of the summed counts
    (loss = summed loss / summed n_valid), 'out_path': out_path or None}
    loss='ce': `predictions/<stem>` receives the uint8 class map, the slides' scores are classify_slide(loss='ce')'s and
    'pooled' is ce_summary of the summed counts and sums (loss = summed loss / summed weight)."""
    if loss not in ("bce", "ce"):
        raise ValueError(f"loss must be 'bce' or 'ce', got {loss!r}")
    ce = loss == "ce"
    if ce:
        _, eps = ce_arguments(clf.n_out, class_weight, label_smoothing)
        pool = [np.zeros((clf.n_out, clf.n_out), np.int64), 0.0, 0.0, 0]      # raw-equivalent counts, weight, loss, n_bad
    r = hdf5.H5Reader(path)
    images = r["images"]
    masks = r["masks"] if "masks" in r.keys() else None
    stems = sorted(images.keys())
    if names is not None:
        missing = [n for n in names if n not in images]
        if missing:
            raise KeyError(f"no images/{missing[0]} in {path}")
        stems = sorted(names)
    slides = OrderedDict()
    tot = [0, 0, 0, 0, 0.0]
    writer = hdf5.H5Writer(out_path) if out_path is not None else None
    try:
        for stem in stems:
            mname = stem + "_mask"
            mask = masks[mname] if masks is not None and mname in masks else None
            if ce:
                res = classify_slide(clf, images[stem], mask, forward_fn=forward_fn, loss="ce", class_weight=class_weight,
                                     label_smoothing=label_smoothing, background_hack=background_hack)
                if writer is not None:
                    writer.create_dataset("predictions", stem, res["class"])
                res.pop("class")
                slides[stem] = res
                if res:
                    pool[0] += res["confusion"]
                    pool[1] += res["weight_sum"]
                    pool[2] += res["loss_sum"]
                    pool[3] += res["n_bad"]
                continue
            res = classify_slide(clf, images[stem], mask, heat=True, pos_weight=pos_weight, forward_fn=forward_fn)
            if writer is not None:
                writer.create_dataset("predictions", stem, res["heat"])
            res.pop("heat")
            slides[stem] = res
            if res:
                for i, k in enumerate(("tp", "fp", "fn", "tn")):
                    tot[i] += res[k]
                tot[4] += res["loss_sum"]
    finally:
        if writer is not None:
            writer.close()
    if ce:
        return {"slides": slides, "pooled": ce_pooled(*pool), "out_path": str(out_path) if out_path is not None else None}
    return {"slides": slides, "pooled": _summary(*tot), "out_path": str(out_path) if out_path is not None else None}
