"""Held-out evaluation of a pretraining model: loss, token accuracy and GO-annotation prediction quality.

The reference's ``pretrain`` docstring promises evaluation metrics, but the two lines that would have
produced predictions are commented out (``ProteinBERT/utils.py:303-304``).  :func:`evaluate_pretrain`
supplies them: per batch of ``(X, Y, W)`` triples (the training loaders' format) it accumulates

* the reference loss and its two terms (``utils.py:293-294``; the paper-semantics NLL for such a model);
* over the positions with ``w_local > 0``: how many there are and how many the local head predicts right
  (``argmax_v P == y``, lowest index on ties), and the same over the *corrupted* positions (input token
  != target);
* over the annotation entries with ``w_global > 0``: a 256-bin histogram of the predicted probability
  for the positives (``y = 1``) and one for the negatives, ``bin = min(255, int(p * 256))``.

On the HIP backend the encoder runs without backward state and the heads are the gradient-free kernels of
:mod:`..ops.eval_heads`; everything accumulates on the device and the host reads it once at the end.  On
the PyTorch backend the same quantities come from ``heads_torch`` with plain torch ops (the oracle of the
GPU tests).

In reference semantics the local numbers depend on how the evaluation set is batched: the local head
normalises every (position, token) over the BATCH axis (``modules.py:277-284``), so a sample's
probabilities -- and its loss and argmax -- change with the samples it shares a batch with.  That is the
reference's behaviour and is not corrected here; keep the evaluation batch size fixed to compare runs.
"""
from __future__ import annotations

import itertools
from typing import Any, Dict, Optional

import torch

from .losses import pretrain_loss_torch
from .step import resolve_compute_dtype

NBIN = 256
# accumulator layout, shared with ops/eval_heads.py (csrc/evalhead.hip eval_fold_kernel)
C_BATCHES, C_SEQS, C_TOK, C_TOK_HIT, C_MASKED, C_MASKED_HIT, C_HIST = 0, 1, 2, 3, 4, 5, 8
N_COUNTS = C_HIST + 2 * NBIN


class _TorchAccumulator:
    """The PyTorch path's accumulator: the same two tensors as ``ops.eval_heads.EvalAccumulator``."""

    def __init__(self, device):
        self.loss = torch.zeros(2, dtype=torch.float64, device=device)
        self.counts = torch.zeros(N_COUNTS, dtype=torch.int64, device=device)


def batch_counts_torch(probs_l: torch.Tensor, probs_g: torch.Tensor, x_local: torch.Tensor,
                       Y: Dict[str, torch.Tensor], W: Dict[str, torch.Tensor]) -> torch.Tensor:
    """int64 [520] counts of one batch from the heads' probabilities (layout of the accumulator)."""
    out = torch.zeros(N_COUNTS, dtype=torch.int64, device=probs_l.device)
    y_l = Y["local"]
    pred = probs_l.argmax(dim=-1)                     # the first maximal index on ties
    counted = W["local"] > 0
    hit = counted & (pred == y_l)
    masked = counted & (x_local != y_l)
    out[C_BATCHES] = 1
    out[C_SEQS] = y_l.shape[0]
    out[C_TOK] = counted.sum()
    out[C_TOK_HIT] = hit.sum()
    out[C_MASKED] = masked.sum()
    out[C_MASKED_HIT] = (masked & hit).sum()
    p = probs_g.float()
    sel = (W["global"] > 0).expand_as(p)
    pos = Y["global"] > 0.5
    bins = (p * NBIN).long().clamp_(max=NBIN - 1)
    out[C_HIST:C_HIST + NBIN] = _hist(bins[sel & pos])
    out[C_HIST + NBIN:] = _hist(bins[sel & ~pos])
    return out


def _hist(bins: torch.Tensor) -> torch.Tensor:
    """Counts of the values 0 .. 255 (sort + searchsorted: ``bincount`` has no deterministic GPU form)."""
    s = bins.reshape(-1).sort().values
    edges = torch.searchsorted(s, torch.arange(NBIN + 1, device=s.device))
    return edges[1:] - edges[:-1]


def _ratio(num: float, den: float) -> float:
    return float(num) / float(den) if den else float("nan")


def metrics_from_accumulator(loss: torch.Tensor, counts: torch.Tensor) -> Dict[str, Any]:
    """The metrics dict from host copies of the accumulator (``loss`` fp64 [2], ``counts`` int64 [520])."""
    c = [int(v) for v in counts.tolist()]
    nb = c[C_BATCHES]
    hp, hn = c[C_HIST:C_HIST + NBIN], c[C_HIST + NBIN:C_HIST + 2 * NBIN]
    npos, nneg = sum(hp), sum(hn)
    half = NBIN // 2                                   # bins >= 128 <=> p >= 0.5 exactly (128 / 256)
    tp, fp = sum(hp[half:]), sum(hn[half:])
    # Mann-Whitney U over the binned scores: a positive outranks every negative in a lower bin and half of
    # those in its own
    below, u = 0, 0.0
    for b in range(NBIN):
        u += hp[b] * (below + 0.5 * hn[b])
        below += hn[b]
    ll, lg = (float(v) for v in loss.tolist())
    return {
        "loss": _ratio(ll + lg, nb), "loss_local": _ratio(ll, nb), "loss_global": _ratio(lg, nb),
        "token_accuracy": _ratio(c[C_TOK_HIT], c[C_TOK]),
        "masked_token_accuracy": _ratio(c[C_MASKED_HIT], c[C_MASKED]),
        "go_precision": _ratio(tp, tp + fp), "go_recall": _ratio(tp, npos),
        "go_f1": _ratio(2 * tp, 2 * tp + fp + (npos - tp)),
        "go_auroc": _ratio(u, float(npos) * float(nneg)),
        "n_batches": nb, "n_sequences": c[C_SEQS], "n_tokens": c[C_TOK], "n_masked_tokens": c[C_MASKED],
        "n_go_pos": npos, "n_go_neg": nneg,
        "go_hist_pos": counts[C_HIST:C_HIST + NBIN].clone(),
        "go_hist_neg": counts[C_HIST + NBIN:C_HIST + 2 * NBIN].clone(),
    }


def scalar_metrics(m: Dict[str, Any]) -> Dict[str, float]:
    """The scalar entries of a metrics dict (what the JSONL / TensorBoard writers take)."""
    return {k: v for k, v in m.items() if not isinstance(v, torch.Tensor)}


def evaluate_pretrain(model, dataloader, max_batches: Optional[int] = None, device=None, compute_dtype="auto",
                      distributed: bool = False) -> Dict[str, Any]:
    """Evaluate ``model`` on up to ``max_batches`` batches of ``dataloader`` (all of them when None: give a
    bound for an endless loader such as the synthetic source).  Runs under ``torch.no_grad()`` with the
    model in ``eval()`` mode and restores the previous mode.  ``distributed``: every rank evaluates its own
    batches and the sums are all-reduced once, so each rank returns the metrics of the whole set.

    Returns ``loss`` / ``loss_local`` / ``loss_global`` (mean over the batches of the per-batch loss),
    ``token_accuracy``, ``masked_token_accuracy`` (over the corrupted positions), ``go_precision`` /
    ``go_recall`` / ``go_f1`` at threshold 0.5, ``go_auroc`` (Mann-Whitney over the 256 score bins, ties
    within a bin counted half), the counts ``n_batches``, ``n_sequences``, ``n_tokens``,
    ``n_masked_tokens``, ``n_go_pos``, ``n_go_neg`` and the raw ``go_hist_pos`` / ``go_hist_neg`` (int64
    [256] CPU tensors).  A metric whose denominator is 0 is ``nan``."""
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    hip = model.resolved_backend(device) == "hip"
    if hip:
        from ..ops.eval_heads import EvalAccumulator, eval_heads
        from ..ops.fused_model import fused_encode
        acc = EvalAccumulator(device)
    else:
        acc = _TorchAccumulator(device)
        dt = resolve_compute_dtype(compute_dtype, device)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for X, Y, W in itertools.islice(iter(dataloader), max_batches):      # draws no batch past the bound
                X, Y, W = ({k: v.to(device, non_blocking=True) for k, v in d.items()} for d in (X, Y, W))
                if hip:
                    h, g, g_bf = fused_encode(model, X["local"], X["global"], return_bf16=True)
                    eval_heads(model, h, g, g_bf, X["local"], Y, W, acc)
                    continue
                h, g = model.encode_torch(X["local"], X["global"], compute_dtype=dt)
                pl, pg = model.heads_torch(h, g)
                Wf = {k: v.float() for k, v in W.items()}
                _, l_local, l_global = pretrain_loss_torch(pl, pg, Y, Wf, model.semantics, return_parts=True)
                acc.loss += torch.stack([l_local, l_global]).double()
                acc.counts += batch_counts_torch(pl, pg, X["local"], Y, Wf)
    finally:
        model.train(was_training)
    if distributed:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            # once per evaluation, not per batch: the fp64 sums and the int64 counts (both exact in their type)
            dist.all_reduce(acc.loss, op=dist.ReduceOp.SUM)
            dist.all_reduce(acc.counts, op=dist.ReduceOp.SUM)
    # the one host read: both tensors in one copy (the fp64 sums travel as their bit patterns)
    host = torch.cat([acc.loss.view(torch.int64), acc.counts]).cpu()
    return metrics_from_accumulator(host[:2].view(torch.float64), host[2:])
