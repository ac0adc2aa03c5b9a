"""Whole-set evaluation of a fine-tuned head: confusion matrix, per-class precision / recall / F1, macro-F1, MCC.

The reference's ``test_step`` (:func:`.finetune.test_step`) reports the mean over batches of a per-batch accuracy:
a short last batch weighs as much as a full one, and accuracy is its only classification metric.
:func:`evaluate_finetune` accumulates exact sums over the whole set instead -- the live rows' cross-entropy in
fp64 and a ``K x K`` confusion matrix in int64, on the device, read by the host once -- and forms every metric
from them (:func:`..ops.task_eval.metrics_from_confusion`).

* :class:`..models.finetune.ProteinBERTForTokenClassification`: one encoder pass per batch; on the HIP backend
  the head is one ``pbx_token_head_eval`` launch whose logits never leave the registers, plus one fold
  (:func:`..ops.task_eval.token_head_eval`); its call of a residue is ``inference.Predictor``'s.  Elsewhere the
  torch definition runs (:func:`..ops.task_eval.token_head_eval_torch`).
* :class:`..models.finetune.ProteinBERTForSequenceClassification` with ``n_classes >= 2``: the ``[B, n]`` logits
  in torch (a few KB per batch); for two classes also ``auroc``, the exact Mann-Whitney statistic of ``P[:, 1]``.
* ``n_classes == 1`` (regression): ``mse``, ``mae``, ``spearman`` and ``pearson`` over the whole set.
"""
from __future__ import annotations

import itertools
from typing import Any, Dict, List, Optional

import torch

from ..models.finetune import (ProteinBERTForSequenceClassification, ProteinBERTForTokenClassification,
                               _split_inputs, encode)
from ..ops import finetune_head, task_eval
from ..ops.task_eval import TaskEvalAccumulator, metrics_from_confusion, scalar_metrics  # noqa: F401
from .finetune import _average_ranks, _to, spearman


def _states(model, X):
    """One encoder pass: ``(hs, gfeat)``: the head's row sources (every block's for ``hidden="all"``, block 0
    first, as ``_encode_all``; else the last block's) and its global feature vector."""
    tokens, ann = _split_inputs(model.encoder, X)
    if model.hidden == "all":
        hs: List[torch.Tensor] = []
        gs: List[torch.Tensor] = []
        encode(model.encoder, tokens, ann, tap=lambda i, h_i, g_i: (hs.append(h_i), gs.append(g_i)))
        return hs, torch.cat([g.float() for g in gs], dim=-1)
    h, g = encode(model.encoder, tokens, ann)
    return [h], g.float()


def _gather_rows(t: torch.Tensor, distributed: bool) -> torch.Tensor:
    """``t`` (a host tensor, rows along dim 0) of every rank, concatenated in rank order."""
    if distributed:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            parts: List[Any] = [None] * dist.get_world_size()
            dist.all_gather_object(parts, t)
            return torch.cat(parts)
    return t


def _ratio(num: float, den: float) -> float:
    return float(num) / float(den) if den else float("nan")


def auroc(scores: torch.Tensor, y: torch.Tensor) -> float:
    """Exact area under the ROC curve of ``scores`` for the labels ``y`` in {0, 1}: the Mann-Whitney statistic
    with average ranks on ties, in fp64; ``nan`` when a class is absent."""
    s, y = scores.reshape(-1).double(), y.reshape(-1)
    pos = y == 1
    npos, nneg = int(pos.sum()), int((y == 0).sum())
    if npos == 0 or nneg == 0:
        return float("nan")
    ranks = _average_ranks(s)
    return (float(ranks[pos].sum()) - npos * (npos + 1) / 2.0) / (float(npos) * float(nneg))


def pearson(pred: torch.Tensor, y: torch.Tensor) -> float:
    """Pearson correlation of two equally long value sets in fp64; ``nan`` when either side is constant."""
    p, t = pred.reshape(-1).double(), y.reshape(-1).double()
    if p.numel() < 2:
        return float("nan")
    p, t = p - p.mean(), t - t.mean()
    den = torch.sqrt((p * p).sum() * (t * t).sum())
    return float((p * t).sum() / den) if den > 0 else float("nan")


def evaluate_finetune(model, dataloader, max_batches: Optional[int] = None, device=None,
                      distributed: bool = False) -> Dict[str, Any]:
    """Evaluate a fine-tuning model on up to ``max_batches`` batches ``(X, y)`` of ``dataloader`` (all of them
    when None).  Runs under ``torch.no_grad()`` with every module in ``eval()`` mode (no backward state, also
    for an unfrozen encoder; dropout is the identity) and restores every module's mode; parameters, gradients
    and optimizer state are untouched.  Nothing is read by the host before the end.

    Classification (per-residue: ``y [B, L]`` with negative labels ignored; per-protein: ``y [B]``): the dict of
    :func:`..ops.task_eval.metrics_from_confusion`, for two per-protein classes with ``auroc`` added.
    Regression (``n_classes == 1``): ``n``, ``mse``, ``mae``, ``spearman``, ``pearson``, ``n_batches``,
    ``n_sequences``.  ``distributed``: the loader is this rank's shard; the sums get one SUM all-reduce and the
    scores / values are gathered, so every rank returns the metrics of the whole set."""
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    token = isinstance(model, ProteinBERTForTokenClassification)
    if not token and not isinstance(model, ProteinBERTForSequenceClassification):
        raise TypeError(f"evaluate_finetune: {type(model).__name__} is not a fine-tuning model of models.finetune")
    K = int(model.n_classes)
    regression = not token and K == 1
    hip = model.encoder.resolved_backend(device) == "hip"
    acc = None if regression else TaskEvalAccumulator(K, device)
    kept_a: List[torch.Tensor] = []             # P[:, 1] (two classes) or the predicted values (regression)
    kept_y: List[torch.Tensor] = []
    nbatch = 0
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            for X, y in itertools.islice(iter(dataloader), max_batches):         # draws no batch past the bound
                X, y = _to(X, device), _to(y, device)
                hs, gfeat = _states(model, X)
                nbatch += 1
                if token:
                    gterm = model.global_head(gfeat) if model.global_head is not None else None     # [B, K]
                    fn = (task_eval.token_head_eval if hip and finetune_head.supported_multi(hs, K)
                          else task_eval.token_head_eval_torch)  # outside the kernel's range (K > 16, C != 128)
                    fn(hs, model.head.weight, model.head.bias, gterm, y.to(torch.int64), acc)
                    continue
                out = model.head(gfeat).float()                                                     # [B, n]
                if regression:
                    kept_a.append(out.reshape(-1))
                    kept_y.append(y.float().reshape(-1))
                    continue
                task_eval.class_counts_into(acc, out, y.reshape(-1))
                if K == 2:
                    kept_a.append(torch.softmax(out, dim=-1)[:, 1])
                    kept_y.append(y.reshape(-1).float())
    finally:
        for m, mode in modes:
            m.training = mode
    both = None
    if kept_a:
        # the one read of the scores / values: both columns in one copy
        both = torch.stack([torch.cat(kept_a).double(), torch.cat(kept_y).double()], dim=1).cpu()
    elif regression or (not token and K == 2):
        both = torch.zeros((0, 2), dtype=torch.float64)
    if both is not None:
        both = _gather_rows(both, distributed)
    if regression:
        p, t = both[:, 0], both[:, 1]
        n = int(p.numel())
        counts = torch.tensor([nbatch, n], dtype=torch.int64, device=device)
        if distributed:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                dist.all_reduce(counts, op=dist.ReduceOp.SUM)
        nb_all = int(counts[0]) if distributed else nbatch
        return {"n": n, "mse": _ratio(float(((p - t) ** 2).sum()), n), "mae": _ratio(float((p - t).abs().sum()), n),
                "spearman": spearman(p, t), "pearson": pearson(p, t), "n_batches": nb_all, "n_sequences": n}
    if distributed:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            # once per evaluation, not per batch: the fp64 sum and the int64 counts (both exact in their type)
            dist.all_reduce(acc.loss, op=dist.ReduceOp.SUM)
            dist.all_reduce(acc.counts, op=dist.ReduceOp.SUM)
    m = metrics_from_confusion(acc)
    if not token and K == 2:
        m["auroc"] = auroc(both[:, 0], both[:, 1])
    return m
