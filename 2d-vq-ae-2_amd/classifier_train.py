"""Training the slide classifier on stored code grids: what validation_nn/train.py does with the HDF5 file
`save_encodings_hdf5` writes, without Lightning and without autograd on the device.

`loss_and_grads` is the whole training step but the optimiser: Camelyon16BCELoss (utils/train_helpers.py:101-138) of
CNNClassifier.step (validation_nn/model.py:131-139) and the gradients of the seven parameter tensors, written to `.grad`, so
any `torch.optim` optimiser over `clf.parameters()` trains the mirror.  On tensors in HBM it is the fused HIP backward
(csrc/classifier_train.hip: no activation tensor is stored); on CPU tensors it is the torch restatement, the same layers
under autograd with F.binary_cross_entropy_with_logits in the parameters' dtype -- the yardstick the tests pin against the
reference's recorded gradients.  `CNNClassifier.train()` and autograd through `CNNClassifier.forward` still raise.

`train_hdf5` walks an archive like the reference's datamodule: `embeddings_split` is CAMELYON16EmbeddingsDataset's choice
and interleaving of the sorted normal* / tumor* / test* slides (datamodules/camelyon16.py:230-246, 287-329),
`collate_random_crop` its collate_unequal_sized_slides (camelyon16.py:381-413), `smooth_targets` the soft targets of the
loss's label smoothing (train_helpers.py:133-135).  The reference's LAMB and SAM optimisers, and the training step that
keeps gradients, optimiser state and weights on the device (ClassifierTrainer), are in optim.py; train_hdf5 takes either.
"""
from itertools import chain, zip_longest

import numpy as np
import torch
import torch.nn.functional as F

from . import hdf5, ops
from .classifier import (_as_codes, _check_codes, _summary, ce_arguments, ce_pooled, ce_stats_host, ce_stats_rows, ce_summary,
                         classify_slide)

PARAM_NAMES = ("embedding.weight", "in_conv.weight", "in_conv.bias", "hidden_conv1.weight", "hidden_conv1.bias",
               "out_conv.weight", "out_conv.bias")


def _params(clf):
    ps = dict(clf.layers.named_parameters())
    return [ps[n] for n in PARAM_NAMES]


def torch_loss_grad(clf, codes, mask, target=None, pos_weight=1.0, reduction="sum"):
    """The torch restatement on the codes' device: the layers of `clf` under autograd and
    F.binary_cross_entropy_with_logits over the codes with mask != 0, in the parameters' dtype.
    -> ([7 gradients in PARAM_NAMES order], (tp, fp, fn, tn, loss_sum))"""
    params = _params(clf)
    dtype = params[0].dtype
    valid = mask != 0
    hard = mask >= 2
    with torch.enable_grad():
        x = clf.reference_forward(codes)[:, 0]
        xv = x[valid]
        t = (hard[valid] if target is None else target[valid]).to(dtype)
        pw = torch.as_tensor(pos_weight, dtype=dtype, device=xv.device)
        loss = F.binary_cross_entropy_with_logits(xv[None], t[None], pos_weight=pw, reduction="sum")
        n = int(valid.sum())
        if reduction == "mean":
            loss = loss / n
        grads = torch.autograd.grad(loss, params, allow_unused=True) if n else [None] * 7
    grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, params)]
    pr, tv = xv.detach() > 0, hard[valid]
    loss_sum = float(loss.detach().double()) * (n if reduction == "mean" else 1)
    return grads, (int((pr & tv).sum()), int((pr & ~tv).sum()), int((~pr & tv).sum()), int((~pr & ~tv).sum()), loss_sum)


def _device_loss_grad(clf, codes, mask, target, pos_weight, reduction):
    """The fused HIP path: packed fp64 gradients split into the seven shapes."""
    loss, packed, stats = clf.native().loss_grad(codes, mask, target=target, pos_weight=pos_weight, reduction=reduction)
    grads, o = [], 0
    for p in _params(clf):
        grads.append(packed[o:o + p.numel()].view(p.shape))
        o += p.numel()
    assert o == packed.numel(), (o, packed.numel())
    rows = stats.cpu().tolist()                                    # counts are exact integers held in doubles
    tp, fp, fn, tn = (int(sum(r[k] for r in rows)) for k in range(4))
    return grads, (tp, fp, fn, tn, float(sum(r[5] for r in rows)))


@torch.no_grad()
def loss_and_grads(clf, codes, mask, *, pos_weight=1.0, reduction="sum", target=None, accumulate=False, grad_fn=None):
    """One training step without the optimiser, for a batch `codes` ([B,H,W], [B,1,H,W] or [H,W], integers as stored) and
    `mask` (same grid; 0 background, 1 tissue, 2 cancer):

      loss_sum = sum over mask != 0 of pos_weight * t * softplus(-x) + (1 - t) * softplus(x),  t = mask - 1, or the soft
      target read from `target` (fp32, same grid, values in [0, 1]; see smooth_targets);
      loss = loss_sum for reduction='sum', loss_sum / n_valid (over the whole batch) for 'mean'.

    Writes d loss / d parameter to `.grad` of clf's seven parameters in their dtype and on their device (adds to an existing
    `.grad` with accumulate=True), so `optimizer.step()` follows; the next call sees the stepped weights (the existing
    handle takes them through vqae_classifier_update).  On tensors in HBM this is the fused HIP backward, on CPU tensors
    the torch restatement (torch_loss_grad); grad_fn(clf, codes, mask, target, pos_weight, reduction) -> (grads, (tp, fp,
    fn, tn, loss_sum)) replaces either, as forward_fn does in classify_slide.
    -> {'loss', 'loss_sum', 'n_valid', 'tp', 'fp', 'fn', 'tn', 'precision', 'recall'}
    ValueError: n_out != 1, shapes that do not match, labels outside 0 .. 2, a target outside [0, 1], reduction='mean' with
    no valid code ('sum' then gives 0 and zero gradients).  IndexError: a code outside the embedding table."""
    if clf.n_out != 1:
        raise ValueError(f"the loss is defined for n_out == 1, this classifier has {clf.n_out}")
    if reduction not in ("sum", "mean"):
        raise ValueError(f"reduction must be 'sum' or 'mean', got {reduction!r}")
    pos_weight = float(pos_weight)
    if not (np.isfinite(pos_weight) and pos_weight >= 0):
        raise ValueError(f"pos_weight must be finite and >= 0, got {pos_weight}")
    codes = _as_codes(codes)
    if mask.dim() == 4 and mask.shape[1] == 1:
        mask = mask[:, 0]
    elif mask.dim() == 2:
        mask = mask[None]
    if tuple(mask.shape) != tuple(codes.shape):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the codes {tuple(codes.shape)}")
    if mask.dtype.is_floating_point:
        raise TypeError(f"the mask holds integer labels, got {mask.dtype}")
    if mask.numel() and (int(mask.min()) < 0 or int(mask.max()) > 2):
        raise ValueError("Camelyon16 labels are 0 (background), 1 (tissue) and 2 (cancer)")
    mask = mask.to(device=codes.device, dtype=torch.uint8)
    if target is not None:
        if target.dim() == 2:
            target = target[None]
        if tuple(target.shape) != tuple(codes.shape):
            raise ValueError(f"target {tuple(target.shape)} does not match the codes {tuple(codes.shape)}")
        target = target.to(device=codes.device, dtype=torch.float32)
        tv = target[mask != 0]
        if tv.numel() and (float(tv.min()) < 0 or float(tv.max()) > 1):
            raise ValueError("soft targets lie in [0, 1]")
    _check_codes(codes, clf.num_embeddings)
    if reduction == "mean" and not bool((mask != 0).any()):
        raise ValueError("reduction='mean' over a batch without a valid code")
    fn_ = grad_fn if grad_fn is not None else (_device_loss_grad if codes.is_cuda else torch_loss_grad)
    grads, (tp, fp, fn, tn, loss_sum) = fn_(clf, codes, mask, target, pos_weight, reduction)
    for p, g in zip(_params(clf), grads):
        g = g.detach().to(device=p.device, dtype=p.dtype)
        if accumulate and p.grad is not None:
            p.grad.add_(g)
        else:
            p.grad = g.clone()
    out = _summary(tp, fp, fn, tn, loss_sum)
    if reduction == "sum":
        out["loss"] = out["loss_sum"]
    return out


# ---- multi-class: nn.CrossEntropyLoss ------------------------------------------------------------------------------------
def torch_ce_loss_grad(clf, codes, labels, class_weight=None, label_smoothing=0.0, reduction="mean"):
    """The torch restatement on the codes' device: the layers of `clf` under autograd and F.cross_entropy(logits [B,NO,H,W],
    labels [B,H,W], weight, label_smoothing, reduction) in the parameters' dtype, as CNNClassifier.step applies
    nn.CrossEntropyLoss (validation_nn/model.py:131-139).
    -> ([7 gradients in PARAM_NAMES order], (confusion [NO,NO] raw counts at [label, prediction], weight_sum, nll_sum,
        smooth_sum, n_bad), loss float)"""
    params = _params(clf)
    dtype = params[0].dtype
    no = clf.n_out
    w = None if class_weight is None else torch.as_tensor(class_weight, dtype=dtype, device=codes.device)
    with torch.enable_grad():
        x = clf.reference_forward(codes)
        loss = F.cross_entropy(x, labels.long(), weight=w, label_smoothing=float(label_smoothing), reduction=reduction)
        grads = torch.autograd.grad(loss, params, allow_unused=True) if labels.numel() else [None] * 7
    grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, params)]
    return grads, ce_stats_host(x.detach(), labels, class_weight, no), float(loss.detach().double())


def _device_ce_loss_grad(clf, codes, labels, class_weight, label_smoothing, reduction):
    """The fused HIP path: packed fp64 gradients split into the seven shapes."""
    loss, packed, stats = clf.native().loss_grad_ce(codes, labels, weight=class_weight, label_smoothing=label_smoothing,
                                                    reduction=reduction)
    grads, o = [], 0
    for p in _params(clf):
        grads.append(packed[o:o + p.numel()].view(p.shape))
        o += p.numel()
    assert o == packed.numel(), (o, packed.numel())
    return grads, ce_stats_rows(stats, clf.n_out), float(loss)


def _as_labels(labels, codes):
    if labels.dim() == 4 and labels.shape[1] == 1:
        labels = labels[:, 0]
    elif labels.dim() == 2:
        labels = labels[None]
    if tuple(labels.shape) != tuple(codes.shape):
        raise ValueError(f"labels {tuple(labels.shape)} do not match the codes {tuple(codes.shape)}")
    if labels.dtype.is_floating_point:
        raise TypeError(f"the labels are integer class indices, got {labels.dtype}")
    return labels


def ce_weight_sum(labels, class_weight, n_out):
    """sum of w[y] over the batch (the 'mean' reduction's divisor), on the host"""
    cnt = torch.bincount(labels.reshape(-1).long(), minlength=n_out)[:n_out].double().cpu()
    return float(cnt.sum()) if class_weight is None else float((cnt * torch.as_tensor(class_weight, dtype=torch.float64)).sum())


@torch.no_grad()
def ce_loss_and_grads(clf, codes, labels, *, class_weight=None, label_smoothing=0.0, reduction="mean", accumulate=False,
                      grad_fn=None, background_hack=True):
    """loss_and_grads for a classifier with n_out = 2 .. 4 and nn.CrossEntropyLoss(weight=class_weight, label_smoothing,
    reduction) (conf/model/loss_f/cross_entropy.yaml): `labels` (the codes' grid, integers) are the stored mask bytes used as
    class indices, and there is no ignore_index -- a position labelled 0 with class_weight[0] == 0 still contributes through
    the smoothing term, as in torch.  Per position with label y and p = softmax(logits):

      loss_sum = (1 - eps) * sum w[y] * -log p_y + (eps / n_out) * sum_c w[c] * -log p_c;  'mean' divides by sum w[y].

    Writes `.grad` as loss_and_grads does (accumulate=True adds).  On tensors in HBM this is the fused HIP path
    (vqae_classifier_loss_grad_ce), on CPU tensors the torch restatement (torch_ce_loss_grad); grad_fn(clf, codes, labels,
    class_weight, label_smoothing, reduction) -> torch_ce_loss_grad's triple replaces either.
    -> {'loss', 'weight_sum', 'confusion', 'precision', 'recall', 'n_bad'} and 'loss_sum': ce_summary's scores, 'loss' being
       the reduction's; background_hack as in classify_slide.
    ValueError: n_out == 1, shapes that do not match, a label >= n_out, a bad class_weight or label_smoothing, reduction=
    'mean' over a zero weight sum.  IndexError: a code outside the embedding table."""
    w, eps = ce_arguments(clf.n_out, class_weight, label_smoothing)
    if reduction not in ("sum", "mean"):
        raise ValueError(f"reduction must be 'sum' or 'mean', got {reduction!r}")
    codes = _as_codes(codes)
    labels = _as_labels(labels, codes)
    if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= clf.n_out):
        raise ValueError(f"labels are class indices 0 .. {clf.n_out - 1}")
    labels = labels.to(device=codes.device, dtype=torch.uint8)
    _check_codes(codes, clf.num_embeddings)
    if reduction == "mean" and not ce_weight_sum(labels, w, clf.n_out) > 0:
        raise ValueError("reduction='mean' over a batch whose class weights sum to zero")
    fn_ = grad_fn if grad_fn is not None else (_device_ce_loss_grad if codes.is_cuda else torch_ce_loss_grad)
    grads, st, loss = fn_(clf, codes, labels, w, eps, reduction)
    for p, g in zip(_params(clf), grads):
        g = g.detach().to(device=p.device, dtype=p.dtype)
        if accumulate and p.grad is not None:
            p.grad.add_(g)
        else:
            p.grad = g.clone()
    out = ce_summary(*st, eps, background_hack)
    out["loss"] = float(loss)
    return out


def smooth_targets(mask, label_smoothing, generator=None):
    """The soft targets of Camelyon16BCELoss's label smoothing (train_helpers.py:133-135) for a whole mask grid:
    |1 - ((1 + t + N(0, 1) * label_smoothing) mod 2)| with t = mask - 1, fp32, on the mask's device, one normal draw per
    code from `generator` (torch.randn of the mask's shape).  Values lie in [0, 1]; those where mask == 0 are never read."""
    t = mask.to(torch.float32) - 1.0
    noise = torch.randn(mask.shape, generator=generator, device=mask.device, dtype=torch.float32)
    return (1.0 - ((1.0 + t + noise * float(label_smoothing)) % 2.0)).abs()


def embeddings_split(keys, train, train_frac):
    """The slide stems CAMELYON16EmbeddingsDataset(train=..., train_frac=...) holds, in its order, out of the keys of
    `images/`: for 'test' the sorted keys that contain 'test'; for 'train' / 'validation' the sorted keys that contain
    'normal' and those that contain 'tumor', each cut at round(n * train_frac) (at least one slide on either side where there
    are two; the first part trains), then interleaved normal, tumor, normal, ... until both run out."""
    if train not in ("train", "validation", "test"):
        raise ValueError(f"train must be 'train', 'validation' or 'test', got {train!r}")
    keys = sorted(str(k) for k in keys)
    if train == "test":
        return [k for k in keys if "test" in k]
    parts = []
    for modality in ("normal", "tumor"):
        ks = [k for k in keys if modality in k]
        ln = len(ks)
        tf = round(ln * train_frac)
        split = tf if 0 < tf < ln else 1 if tf == 0 else tf - 1
        parts.append(ks[:split] if train == "train" else ks[split:ln])
    return [k for k in chain.from_iterable(zip_longest(*parts)) if k is not None]


def collate_random_crop(slides, rng, aligned=False):
    """collate_unequal_sized_slides(mode='random_crop') (camelyon16.py:381-413): slides is a sequence of tuples of arrays
    (code grid, mask, ...); every member of the batch is cropped to the smallest extent of its kind along each axis, at an
    offset drawn as `rng.randint(residuals + 1)` -- the numbers np.random.randint gives the reference from the same state --
    and the crops are stacked -> a tuple of tensors.  As in the reference, each kind draws its OWN offsets: a grid and its
    mask are cropped at different places whenever the batch holds slides of different sizes.  aligned=True crops every kind
    at the offsets drawn for the first instead (one draw per batch)."""
    out, first = [], None
    for arrays in zip(*slides):
        arrays = [np.asarray(a) for a in arrays]
        shape = np.asarray([a.shape for a in arrays])
        residuals = shape - shape.min(axis=0)
        if aligned and first is not None and first[1].shape == residuals.shape and (first[1] == residuals).all():
            start = first[0]
        else:
            start = rng.randint(residuals + 1)
            if first is None:
                first = (start, residuals)
        stop = start - residuals
        crops = [a[tuple(slice(int(s), None if e == 0 else int(e)) for s, e in zip(st, sp))]
                 for a, st, sp in zip(arrays, start, stop)]
        out.append(torch.as_tensor(np.stack(crops)))
    return tuple(out)


def _load_slide(images, masks, stem):
    img, msk = np.asarray(images[stem]), np.asarray(masks[stem + "_mask"])
    if img.dtype == np.bool_:
        img = img.astype(np.uint8)
    if msk.dtype == np.bool_:
        msk = msk.astype(np.uint8)
    return img, msk


def train_hdf5(clf, path, optimizer, *, epochs, batch_size, seed, pos_weight=None, train_frac=0.9, label_smoothing=0.0,
               reduction="sum", shuffle=False, drop_last=False, aligned_crops=False, grad_fn=None, forward_fn=None,
               class_weight=None):
    """Train `clf` on an archive written by save_encodings_hdf5 (`images/<stem>`, `masks/<stem>_mask`) the way the
    reference's datamodule walks it: the training slides of embeddings_split(keys, 'train', train_frac) in that order
    (shuffle=True permutes them per epoch with the seeded RandomState, as the reference's DataLoader shuffles with torch's),
    batch_size at a time through collate_random_crop, one loss_and_grads + optimizer.step() per batch; after each epoch the
    validation slides, whole and one at a time (the reference validates with batch_size 1), through classify_slide.
    seed seeds the crops (numpy RandomState) and the label-smoothing noise (a torch.Generator on the codes' device).
    The batches run on the GPU; grad_fn / forward_fn replace the HIP paths (see loss_and_grads, classify_slide) and keep the
    tensors on the host.
    optimizer may also be the SAM mirror (optim.SAM): each batch is then loss_and_grads, first_step, loss_and_grads again
    (with label smoothing on newly drawn targets, as the reference's loss draws new noise on its second call), second_step,
    and the step's record is the first pass's.  Or a ClassifierTrainer made from `clf` (optim.py): its step runs each batch
    without the host in between (on the CPU when the trainer was built with device='cpu'), losses and stats are read back
    once per epoch, and `clf` receives the weights (sync_to_module) before each epoch's validation.
    -> [{'epoch', 'steps': [{'stems', 'shape', loss_and_grads' dict ...}], 'train': pooled scores of the epoch's steps,
         'val': pooled scores of the validation slides}, ...]   (loss = summed loss / summed n_valid, precision, recall)
    A classifier with n_out > 1 trains with nn.CrossEntropyLoss(weight=class_weight, label_smoothing) instead: the masks go
    in as class indices, label_smoothing is the loss's deterministic eps (no noise is drawn), pos_weight is not used, each
    step is ce_loss_and_grads (or the step of a ClassifierTrainer built with loss='ce', whose class_weight and
    label_smoothing then apply), validation is classify_slide(loss='ce'), and the pooled scores are ce_summary's.
    ValueError: n_out == 1 without pos_weight."""
    if clf.n_out > 1:
        return _train_hdf5_ce(clf, path, optimizer, epochs=epochs, batch_size=batch_size, seed=seed, train_frac=train_frac,
                              label_smoothing=label_smoothing, reduction=reduction, shuffle=shuffle, drop_last=drop_last,
                              aligned_crops=aligned_crops, grad_fn=grad_fn, forward_fn=forward_fn, class_weight=class_weight)
    if pos_weight is None:
        raise ValueError("train_hdf5: pos_weight is required for n_out == 1")
    r = hdf5.H5Reader(path)
    if "images" not in r.keys() or "masks" not in r.keys():
        raise KeyError(f"{path} needs the groups images/ and masks/")
    images, masks = r["images"], r["masks"]
    train_stems = embeddings_split(images.keys(), "train", train_frac)
    val_stems = embeddings_split(images.keys(), "validation", train_frac)
    for s in train_stems + val_stems:
        if s + "_mask" not in masks:
            raise KeyError(f"no masks/{s}_mask in {path}")
    from .optim import SAM, ClassifierTrainer                       # (optim.py imports this module)
    trainer = optimizer if isinstance(optimizer, ClassifierTrainer) else None
    sam = isinstance(optimizer, SAM)
    if trainer is not None:
        if trainer.clf is not clf:
            raise ValueError("train_hdf5: the ClassifierTrainer was made from another classifier")
        if grad_fn is not None:
            raise ValueError("train_hdf5: a ClassifierTrainer computes its own gradients; grad_fn does not apply")
        if trainer.device is None:
            trainer._ensure("cuda")
    on_gpu = grad_fn is None if trainer is None else trainer.device == "cuda"
    rng = np.random.RandomState(seed)
    gen = None
    if label_smoothing:
        gen = torch.Generator(device="cuda" if on_gpu else "cpu")
        gen.manual_seed(int(seed))
    history = []
    for epoch in range(int(epochs)):
        order = list(train_stems)
        if shuffle:
            order = [order[i] for i in rng.permutation(len(order))]
        steps, tot = [], [0, 0, 0, 0, 0.0]
        for i in range(0, len(order), batch_size):
            stems = order[i:i + batch_size]
            if drop_last and len(stems) < batch_size:
                break
            codes, mask = collate_random_crop([_load_slide(images, masks, s) for s in stems], rng, aligned=aligned_crops)
            if codes.dtype not in ops._IDX_DTYPES:
                codes = codes.to(torch.int32)
            mask = mask.to(torch.uint8)
            if on_gpu:
                codes, mask = codes.cuda(), mask.cuda()
            target = smooth_targets(mask, label_smoothing, gen) if label_smoothing else None
            if trainer is not None:
                target2 = smooth_targets(mask, label_smoothing, gen) if label_smoothing and trainer.sam_rho is not None else None
                steps.append((trainer.step(codes, mask, pos_weight=pos_weight, reduction=reduction, target=target,
                                           target2=target2), list(stems), tuple(codes.shape)))
                continue
            optimizer.zero_grad(set_to_none=True)
            res = loss_and_grads(clf, codes, mask, pos_weight=pos_weight, reduction=reduction, target=target, grad_fn=grad_fn)
            if sam:
                optimizer.first_step(zero_grad=True)
                target = smooth_targets(mask, label_smoothing, gen) if label_smoothing else None
                loss_and_grads(clf, codes, mask, pos_weight=pos_weight, reduction=reduction, target=target, grad_fn=grad_fn)
                optimizer.second_step(zero_grad=True)
            else:
                optimizer.step()
            steps.append(dict(res, stems=list(stems), shape=tuple(codes.shape)))
            for j, k in enumerate(("tp", "fp", "fn", "tn", "loss_sum")):
                tot[j] += res[k]
        if trainer is not None:
            if steps:                                              # the epoch's one read-back: every step's pooled stats row
                rows = torch.stack([st.sum(0) for (_, st), _, _ in steps]).cpu().tolist()
                for n, r in enumerate(rows):
                    res = _summary(int(r[0]), int(r[1]), int(r[2]), int(r[3]), r[5])
                    if reduction == "sum":
                        res["loss"] = res["loss_sum"]
                    for j, k in enumerate(("tp", "fp", "fn", "tn", "loss_sum")):
                        tot[j] += res[k]
                    steps[n] = dict(res, stems=steps[n][1], shape=steps[n][2])
            trainer.sync_to_module()
        vtot = [0, 0, 0, 0, 0.0]
        for s in val_stems:
            img, msk = _load_slide(images, masks, s)
            res = classify_slide(clf, img, msk, heat=False, pos_weight=pos_weight, forward_fn=forward_fn)
            for j, k in enumerate(("tp", "fp", "fn", "tn", "loss_sum")):
                vtot[j] += res[k]
        history.append({"epoch": epoch, "steps": steps, "train": _summary(*tot), "val": _summary(*vtot)})
    return history


def _train_hdf5_ce(clf, path, optimizer, *, epochs, batch_size, seed, train_frac, label_smoothing, reduction, shuffle, drop_last,
                   aligned_crops, grad_fn, forward_fn, class_weight):
    """train_hdf5 for n_out > 1 (see there)"""
    r = hdf5.H5Reader(path)
    if "images" not in r.keys() or "masks" not in r.keys():
        raise KeyError(f"{path} needs the groups images/ and masks/")
    images, masks = r["images"], r["masks"]
    train_stems = embeddings_split(images.keys(), "train", train_frac)
    val_stems = embeddings_split(images.keys(), "validation", train_frac)
    for s in train_stems + val_stems:
        if s + "_mask" not in masks:
            raise KeyError(f"no masks/{s}_mask in {path}")
    from .optim import SAM, ClassifierTrainer                       # (optim.py imports this module)
    trainer = optimizer if isinstance(optimizer, ClassifierTrainer) else None
    sam = isinstance(optimizer, SAM)
    if trainer is not None:
        if trainer.clf is not clf:
            raise ValueError("train_hdf5: the ClassifierTrainer was made from another classifier")
        if trainer.loss != "ce":
            raise ValueError("train_hdf5: a classifier with n_out > 1 needs a ClassifierTrainer built with loss='ce'")
        if grad_fn is not None:
            raise ValueError("train_hdf5: a ClassifierTrainer computes its own gradients; grad_fn does not apply")
        if trainer.device is None:
            trainer._ensure("cuda")
        class_weight, label_smoothing = trainer.class_weight, trainer.label_smoothing
    w, eps = ce_arguments(clf.n_out, class_weight, label_smoothing)
    no = clf.n_out
    on_gpu = grad_fn is None if trainer is None else trainer.device == "cuda"
    rng = np.random.RandomState(seed)
    kw = dict(class_weight=w, label_smoothing=eps)

    history = []
    for epoch in range(int(epochs)):
        order = list(train_stems)
        if shuffle:
            order = [order[i] for i in rng.permutation(len(order))]
        steps, tot = [], [np.zeros((no, no), np.int64), 0.0, 0.0, 0]
        for i in range(0, len(order), batch_size):
            stems = order[i:i + batch_size]
            if drop_last and len(stems) < batch_size:
                break
            codes, labels = collate_random_crop([_load_slide(images, masks, s) for s in stems], rng, aligned=aligned_crops)
            if codes.dtype not in ops._IDX_DTYPES:
                codes = codes.to(torch.int32)
            labels = labels.to(torch.uint8)
            if on_gpu:
                codes, labels = codes.cuda(), labels.cuda()
            if trainer is not None:
                steps.append((trainer.step(codes, labels, reduction=reduction), list(stems), tuple(codes.shape)))
                continue
            optimizer.zero_grad(set_to_none=True)
            res = ce_loss_and_grads(clf, codes, labels, reduction=reduction, grad_fn=grad_fn, **kw)
            if sam:
                optimizer.first_step(zero_grad=True)
                ce_loss_and_grads(clf, codes, labels, reduction=reduction, grad_fn=grad_fn, **kw)
                optimizer.second_step(zero_grad=True)
            else:
                optimizer.step()
            steps.append(dict(res, stems=list(stems), shape=tuple(codes.shape)))
        if trainer is not None:
            for n, ((loss, st), stems, shape) in enumerate(steps):  # read back after the epoch's last step was queued
                res = ce_summary(*ce_stats_rows(st, no), eps)
                res["loss"] = float(loss)
                steps[n] = dict(res, stems=stems, shape=shape)
            trainer.sync_to_module()
        for res in steps:
            tot[0] += res["confusion"]
            tot[1] += res["weight_sum"]
            tot[2] += res["loss_sum"]
            tot[3] += res["n_bad"]
        vtot = [np.zeros((no, no), np.int64), 0.0, 0.0, 0]
        for s in val_stems:
            img, msk = _load_slide(images, masks, s)
            res = classify_slide(clf, img, msk, loss="ce", forward_fn=forward_fn, **kw)
            vtot[0] += res["confusion"]
            vtot[1] += res["weight_sum"]
            vtot[2] += res["loss_sum"]
            vtot[3] += res["n_bad"]
        history.append({"epoch": epoch, "steps": steps, "train": ce_pooled(*tot), "val": ce_pooled(*vtot)})
    return history
