"""Counting stored code grids: the exact code and label histograms the reference commits as data under
scripts/create_wsi_histograms/ (embedding_idx_histogram_{K}_{split}.npy, histogram_{split}.npy; it ships no program that
produces them), and what it derives from them -- the perplexity / dead codes of a codebook (the commented-out health check
of EMAVectorQuantizer.forward, vq.py:135-136) and the loss weights of
conf/model/optional_overrides/loss_f/{bce_with_logits_loss,cross_entropy}_camelyon16_embeddings.yaml ("values taken from
validation marginal").

On tensors in HBM the counting is one HIP pass in exact integers (csrc/code_stats.hip, ops.code_histogram); on CPU tensors
and arrays it is the numpy restatement (host_code_histogram), the yardstick of the tests.  hist_fn= replaces the device
path of the archive driver the way forward_fn / grad_fn do elsewhere; it takes ops.code_histogram's arguments.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import hdf5, ops
from .classifier import _grid_tensor
from .classifier_train import embeddings_split

LABEL_NAMES = ("background", "tissue", "cancer")
_SPLIT_FILE = {"train": "train", "validation": "val", "test": "test"}      # histogram_{train,val,test}.npy


def _np(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu()
        return t.to(torch.int32).numpy() if t.dtype == getattr(torch, "uint16", None) else t.numpy()
    return np.asarray(t)


def host_code_histogram(codes, mask=None, *, num_embeddings, n_labels=None, pooled=False, out=None, bad=None):
    """The numpy restatement of ops.code_histogram, same arguments and results on CPU tensors: np.bincount of
    label * K + code over the positions whose code lies in 0 .. K-1 and whose label is < n_labels; the others are counted in
    bad[:, 0] (code) and bad[:, 1] (label, code in range)."""
    c = _np(codes)
    B = c.shape[0]
    c = c.reshape(B, -1).astype(np.int64)
    if n_labels is None:
        n_labels = 3 if mask is not None else 1
    K, L = int(num_embeddings), int(n_labels)
    m = _np(mask).reshape(B, -1).astype(np.int64) if mask is not None else np.zeros_like(c)
    hist = np.zeros((B, L, K), np.int64)
    bd = np.zeros((B, 2), np.int64)
    for b in range(B):
        ok = (c[b] >= 0) & (c[b] < K)
        okl = m[b] < L
        v = ok & okl
        hist[b] = np.bincount(m[b][v] * K + c[b][v], minlength=L * K).reshape(L, K)
        bd[b] = ((~ok).sum(), (ok & ~okl).sum())
    if pooled:
        hist, bd = hist.sum(0, keepdims=True), bd.sum(0, keepdims=True)
    hist, bd = torch.from_numpy(hist), torch.from_numpy(bd)
    if out is not None or bad is not None:
        out = hist if out is None else out.add_(hist)
        bad = bd if bad is None else bad.add_(bd)
        return out, bad
    return hist, bd


def perplexity(counts):
    """exp(-sum p * log(p + 1e-10)) with p = counts / counts.sum() in fp64: the perplexity of vq.py:135-136
    (`avg_probs = encodings.mean(0)`) from integer counts.  An empty histogram gives nan."""
    c = np.asarray(counts, np.float64).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = c / c.sum()
    return float(np.exp(-np.sum(p * np.log(p + 1e-10))))


def class_weights(labels, decimals=None):
    """[background, tissue, cancer] counts -> what the reference's loss YAMLs derive from them, unrounded fp64:
      'marginal'   P(background), P(tissue), P(cancer);
      'foreground' P(tissue), P(cancer) among the positions that are not background;
      'ce_weight'  [0, P(cancer | fg), P(tissue | fg)]       (cross_entropy_camelyon16_embeddings.yaml `weight`);
      'reciprocal' 1 / marginal                               (that file's commented alternative);
      'pos_weight' (tissue + cancer) / cancer = 1 / P(cancer | fg)   (bce_with_logits_loss_camelyon16_embeddings.yaml).
    decimals=4 reproduces the reference's figures: the probabilities are rounded to that many decimals first, and the
    reciprocals are taken of the rounded values.  A count of zero gives inf (or nan for 0 / 0), never an exception."""
    c = np.asarray(labels, np.float64).reshape(-1)
    if c.shape != (3,):
        raise ValueError(f"class_weights takes [background, tissue, cancer] counts, got shape {np.shape(labels)}")
    with np.errstate(invalid="ignore", divide="ignore"):
        marginal = c / c.sum()
        fg = c[1:] / (c[1] + c[2])
        if decimals is not None:
            marginal, fg = np.round(marginal, decimals), np.round(fg, decimals)
            pos_weight = float(np.float64(1.0) / fg[1])
        else:
            pos_weight = float((c[1] + c[2]) / c[2])
        reciprocal = 1.0 / marginal
    return {"marginal": marginal, "foreground": fg, "ce_weight": np.array([0.0, fg[1], fg[0]]), "reciprocal": reciprocal,
            "pos_weight": pos_weight}


def _result(joint, codes=None):
    """joint [n_labels][K] (or None with codes [K] for a grid without labels) -> the dict code_histogram returns"""
    if joint is not None:
        joint = np.ascontiguousarray(joint, np.int64)
        codes, labels = joint.sum(0), joint.sum(1)
    else:
        codes, labels = np.ascontiguousarray(codes, np.int64), None
    return {"joint": joint, "codes": codes, "labels": labels, "n": int(codes.sum()), "perplexity": perplexity(codes),
            "dead": int((codes == 0).sum())}


def _raise_bad(bad, num_embeddings, what):
    """IndexError for codes outside the table (as nn.Embedding and classifier._check_codes), ValueError for labels above 2
    (as Camelyon16BCELoss, utils/train_helpers.py:116-120), from the kernel's own `bad` counters."""
    if int(bad[0]):
        raise IndexError(f"index out of range in self: {int(bad[0])} codes of {what} lie outside 0 .. {num_embeddings - 1}")
    if int(bad[1]):
        raise ValueError("Camelyon16 Targets values are assumed to be 0 (background), 1 (tissue) and 2 (cancer)."
                         f" Instead, found {int(bad[1])} other labels in {what}")


def _as_grid(a, what):
    """array as stored / tensor of any rank -> integer tensor (bool -> uint8, widths the kernel does not take widened)"""
    if isinstance(a, torch.Tensor):
        if a.dtype.is_floating_point or a.dtype.is_complex:
            raise TypeError(f"{what} must hold integers, got {a.dtype}")
        if a.dtype == torch.bool:
            a = a.to(torch.uint8)
        elif a.dtype not in ops._IDX_DTYPES:
            a = a.to(torch.int32 if a.element_size() <= 2 else torch.int64)
        return a
    a = np.asarray(a)
    return _grid_tensor(a.reshape(1, -1), what).reshape(a.shape)


def _as_mask(m, what):
    """integer tensor -> uint8.  Labels 3 .. 255 are left to the kernel's own `bad` counter; only a wider dtype can hold a
    value the cast would fold into range, and only then is there a min / max pass."""
    if m.dtype != torch.uint8:
        if m.numel() and (int(m.min()) < 0 or int(m.max()) > 255):
            raise ValueError("Camelyon16 Targets values are assumed to be 0 (background), 1 (tissue) and 2 (cancer)."
                             f" Instead, found values outside 0 .. 255 in {what}")
        m = m.to(torch.uint8)
    return m


@torch.no_grad()
def code_histogram(grid, mask=None, *, num_embeddings, hist_fn=None):
    """One code grid (array as stored or tensor, any shape) and optionally its mask (0 background, 1 tissue, 2 cancer) ->
      'joint'  int64 [n_labels][K], joint[l][k] = positions with mask == l and code == k (n_labels = 3 with a mask, else 1);
      'codes'  int64 [K] = joint.sum(0);  'labels' int64 [n_labels] = joint.sum(1);  'n' their total;
      'perplexity' of `codes` (see perplexity);  'dead' the number of codes that never occur.
    A tensor in HBM is counted by the HIP kernel, a CPU tensor or an array by the numpy restatement; hist_fn (the arguments
    of ops.code_histogram) replaces either.
    IndexError: a code outside 0 .. num_embeddings-1.  ValueError: a label above 2, a mask of another shape."""
    g = _as_grid(grid, "code grid")
    m = None
    if mask is not None:
        m = _as_grid(mask, "mask")
        if tuple(m.shape) != tuple(g.shape):
            raise ValueError(f"mask {tuple(m.shape)} does not match the code grid {tuple(g.shape)}")
        m = _as_mask(m, "the mask").to(g.device).reshape(1, -1)
    K = int(num_embeddings)
    if g.numel() == 0:
        return _result(np.zeros((3 if m is not None else 1, K), np.int64))
    fn = hist_fn if hist_fn is not None else (ops.code_histogram if g.is_cuda else host_code_histogram)
    hist, bad = fn(g.reshape(1, -1), m, num_embeddings=K, n_labels=3 if m is not None else 1)
    hist, bad = _np(hist), _np(bad)
    _raise_bad(bad[0], K, "the grid")
    return _result(hist[0])


def _next_pow2(n):
    return 1 << max(0, int(n) - 1).bit_length()


@torch.no_grad()
def histogram_hdf5(path, *, split=None, train_frac=0.9, names=None, num_embeddings=None, out_dir=None, hist_fn=None):
    """Count an archive written by save_encodings_hdf5 / convert_npy_to_hdf5 (`images/<stem>`, `masks/<stem>_mask`).
      split         None: every slide in sorted key order; 'train' / 'validation' / 'test': the slides and order of
                    embeddings_split(keys, split, train_frac), the reference's dataset;
      names         the stems to take (of the split).  Only a slide NAMED here may lack its mask: it is then counted without
                    labels (it enters 'codes', not 'joint' / 'labels'); otherwise a missing mask raises KeyError, as in
                    train_hdf5;
      num_embeddings  the table size K.  Default: max code + 1 over the chosen slides, rounded up to a power of two -- found
                    by a first pass of np.max over the arrays on the host (the dtype's range would make every uint16 archive
                    a 65536-bin table); only the default pays for that pass;
      out_dir       receives the reference's files under the reference's names, int64:
                    embedding_idx_histogram_{K}_{train|validation|test}.npy (K,), histogram_{train|val|test}.npy (3,), and
                    joint_histogram_{K}_{split}.npy (3, K), which the reference lacks.  Without a split the names end in
                    `_all` and the labels go to camelyon16_mask_histogram_bg_tissue_cancer.npy, the reference's name for the
                    whole dataset.
    Each slide is uploaded and counted into its own row of ONE device table (the kernel adds into the row: `accumulate`); no
    synchronisation per slide, one download at the end; the pooled counts are the sum of the rows.  hist_fn (the arguments
    of ops.code_histogram) replaces the HIP path and keeps the tensors on the host.
    -> {'split', 'num_embeddings', 'stems', 'slides': {stem: code_histogram's dict, 'joint' / 'labels' None without a mask},
        'pooled': code_histogram's dict over all slides ('joint' / 'labels' over those with a mask), 'files': [paths]}
    IndexError / ValueError as code_histogram, naming the slide."""
    r = hdf5.H5Reader(path)
    if "images" not in r.keys():
        raise KeyError(f"{path} needs the group images/")
    images = r["images"]
    masks = r["masks"] if "masks" in r.keys() else None
    if split is None:
        stems = sorted(str(k) for k in images.keys())
    else:
        stems = embeddings_split(images.keys(), split, train_frac)
    if names is not None:
        names = [str(n) for n in names]
        missing = [n for n in names if n not in images]
        if missing:
            raise KeyError(f"no images/{missing[0]} in {path}")
        stems = [s for s in stems if s in set(names)]
    has_mask = []
    for s in stems:
        ok = masks is not None and s + "_mask" in masks
        if not ok and names is None:
            raise KeyError(f"no masks/{s}_mask in {path}")
        has_mask.append(ok)

    grids = None
    if num_embeddings is None:
        grids = [np.asarray(images[s]) for s in stems]            # the first pass keeps what it read
        top = max((int(g.max()) for g in grids if g.size), default=0)
        num_embeddings = _next_pow2(top + 1)
    K = int(num_embeddings)
    fn = hist_fn if hist_fn is not None else ops.code_histogram
    dev = "cuda" if hist_fn is None else "cpu"
    # one int64 row per slide: [3 * K joint bins | bad codes, bad labels]; a slide without a mask uses the first K bins
    table = torch.zeros((len(stems), 3 * K + 2), dtype=torch.int64, device=dev)
    for i, s in enumerate(stems):
        g = _as_grid(grids[i] if grids is not None else images[s], f"images/{s}").reshape(1, -1)
        if g.numel() == 0:
            continue
        L = 3 if has_mask[i] else 1
        m = None
        if has_mask[i]:
            m = _as_grid(masks[s + "_mask"], f"masks/{s}_mask")
            if m.numel() != g.numel():
                raise ValueError(f"masks/{s}_mask {tuple(m.shape)} does not match images/{s}")
            m = _as_mask(m, f"masks/{s}_mask").reshape(1, -1).to(dev)
        fn(g.to(dev), m, num_embeddings=K, n_labels=L, out=table[i, :L * K].view(1, L, K), bad=table[i, 3 * K:].view(1, 2))
    rows = table.cpu().numpy()                                     # the one download (and the one synchronisation)

    slides = OrderedDict()
    joint, codes = np.zeros((3, K), np.int64), np.zeros(K, np.int64)
    for i, s in enumerate(stems):
        _raise_bad(rows[i, 3 * K:], K, f"images/{s}")
        if has_mask[i]:
            res = _result(rows[i, :3 * K].reshape(3, K))
            joint += res["joint"]
        else:
            res = _result(None, rows[i, :K])
        codes += res["codes"]
        slides[s] = res
    pooled = _result(joint)
    if not all(has_mask):
        pooled.update(codes=codes, n=int(codes.sum()), perplexity=perplexity(codes), dead=int((codes == 0).sum()))

    files = []
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        tag = split if split is not None else "all"
        lab = f"histogram_{_SPLIT_FILE[split]}.npy" if split is not None else "camelyon16_mask_histogram_bg_tissue_cancer.npy"
        for name, arr in ((f"embedding_idx_histogram_{K}_{tag}.npy", pooled["codes"]), (lab, pooled["labels"]),
                          (f"joint_histogram_{K}_{tag}.npy", pooled["joint"])):
            p = os.path.join(str(out_dir), name)
            np.save(p, np.ascontiguousarray(arr, np.int64))
            files.append(p)
    return {"split": split, "num_embeddings": K, "stems": list(stems), "slides": slides, "pooled": pooled, "files": files}


@torch.no_grad()
def label_histogram_hdf5(path, *, split=None, train_frac=0.9, hist_fn=None):
    """[background, tissue, cancer] counts (int64 [3]) of the masks of one split: the masks alone are read, uploaded and
    counted -- each as a uint8 'code' grid into one pooled 3-bin device table, any other label landing in the kernel's `bad`
    counter -- so the cost is one byte per position; the code grids are not touched.  One download at the end.
    KeyError: a slide of the split without its mask.  ValueError: a label above 2."""
    r = hdf5.H5Reader(path)
    if "images" not in r.keys() or "masks" not in r.keys():
        raise KeyError(f"{path} needs the groups images/ and masks/")
    images, masks = r["images"], r["masks"]
    stems = sorted(str(k) for k in images.keys()) if split is None else embeddings_split(images.keys(), split, train_frac)
    for s in stems:
        if s + "_mask" not in masks:
            raise KeyError(f"no masks/{s}_mask in {path}")
    fn = hist_fn if hist_fn is not None else ops.code_histogram
    dev = "cuda" if hist_fn is None else "cpu"
    table = torch.zeros(5, dtype=torch.int64, device=dev)              # 3 label bins, then the two `bad` counters
    for s in stems:
        m = _as_mask(_as_grid(masks[s + "_mask"], f"masks/{s}_mask"), f"masks/{s}_mask").reshape(1, -1)
        if m.numel():
            fn(m.to(dev), None, num_embeddings=3, n_labels=1, pooled=True, out=table[:3].view(1, 1, 3), bad=table[3:].view(1, 2))
    counts = table.cpu().numpy()
    if int(counts[3]):
        raise ValueError("Camelyon16 Targets values are assumed to be 0 (background), 1 (tissue) and 2 (cancer)."
                         f" Instead, found {int(counts[3])} other labels in the masks of {path}")
    return np.ascontiguousarray(counts[:3])


def pos_weight_hdf5(path, split="validation", train_frac=0.9, *, hist_fn=None):
    """The `pos_weight` to hand to train_hdf5: (tissue + cancer) / cancer over the masks of one split of the archive (the
    reference took its 40.4858 from the validation marginal); inf for a split without cancer.  Only the masks are counted
    (label_histogram_hdf5): one byte per position, no pass over the codes."""
    return class_weights(label_histogram_hdf5(path, split=split, train_frac=train_frac, hist_fn=hist_fn))["pos_weight"]
