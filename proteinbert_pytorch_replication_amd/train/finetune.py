"""Fine-tuning loops (reference ``train_step`` / ``test_step``, ``ProteinBERT/utils.py:110-217``, T2/T3).

Same signatures and return values as the reference - ``(mean_loss, {metric_name: mean_value})`` per
epoch, metrics called as ``metric(softmax(logits, dim=1), y)`` - with these MI355X-side changes:

* no host sync per batch: loss and metric sums accumulate on the device and are read once at the
  end of the epoch (the reference calls ``loss.item()`` and ``.numpy()`` every batch);
* gradient clipping uses the fused arena grad-norm kernel when the optimizer is
  :class:`.optim.FusedAdam`, else ``torch.nn.utils.clip_grad_norm_``;
* ``X`` may be a tensor or the pretraining-style dict; ``(X, y)`` batches go to ``device`` with
  ``non_blocking`` copies;
* under data parallelism (``ddp`` given) gradients are all-reduced through the bucketed RCCL
  reducer before the optimizer step and the epoch means are averaged over ranks;
* a :class:`.task_loss.ResidueTaskLoss` (class weights, label smoothing) on a model with a ``loss`` method is
  taken through ``model.loss(X, y, loss_fn)``: on a GPU one HIP launch computes the head, the loss, the
  accuracy and the logit gradient, and the logits never reach memory (:func:`_fused_loss_step`).
"""
from __future__ import annotations

from typing import Any, Callable, Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from ..parallel import dist as pdist
from .optim import FusedAdam
from .task_loss import N_BAD, ResidueTaskLoss


def _to(x, device):
    if isinstance(x, dict):
        return {k: v.to(device, non_blocking=True) for k, v in x.items()}
    return x.to(device, non_blocking=True)


def _metric_value(v) -> torch.Tensor:
    if isinstance(v, torch.Tensor):
        return v.detach().float().reshape(())
    return torch.tensor(float(v))


def _default_device():
    return "cuda" if torch.cuda.is_available() else "cpu"


def train_step(model: torch.nn.Module, dataloader, loss_fn: torch.nn.Module, optimizer: torch.optim.Optimizer,
               metrics: Dict[str, Callable], gradient_clipping: bool = True, gradient_clipping_thresh: float = 1,
               device=None, ddp=None) -> Tuple[float, Dict[str, float]]:
    device = torch.device(device or _default_device())
    model.train()
    loss_sum = torch.zeros((), dtype=torch.float32, device=device)
    met_sum = {k: torch.zeros((), dtype=torch.float32, device=device) for k in metrics}
    n = 0
    fused = isinstance(optimizer, FusedAdam)
    params = [p for p in model.parameters() if p.requires_grad]
    by_model = _fused_loss_step(model, loss_fn, metrics)
    if by_model:
        loss_fn.counter(device).zero_()
    for X, y in dataloader:
        X, y = _to(X, device), _to(y, device)
        if by_model:
            loss, acc = model.loss(X, y, loss_fn)
        else:
            logits = model(X)
            loss = loss_fn(logits, y)
        loss_sum += loss.detach().float()
        optimizer.zero_grad()
        loss.backward()
        if ddp is not None:
            ddp.finish(average=not fused)
        if gradient_clipping:
            if fused:
                optimizer.clip_grad_norm_(gradient_clipping_thresh)
            else:
                torch.nn.utils.clip_grad_norm_(params, gradient_clipping_thresh)
        optimizer.step()
        if by_model:
            for k in metrics:
                met_sum[k] += acc.detach().float()
        elif metrics:
            with torch.no_grad():
                preds = torch.softmax(logits.detach().float(), dim=1)
                for k, m in metrics.items():
                    met_sum[k] += _metric_value(m(preds, y)).to(device)
        n += 1
    return _finish(loss_sum, met_sum, n, ddp is not None, loss_fn.counter(device) if by_model else None)


def _fused_loss_step(model, loss_fn, metrics) -> bool:
    """Whether :func:`train_step` takes ``model.loss(X, y, loss_fn)``: a :class:`.task_loss.ResidueTaskLoss`, a
    model that has ``loss``, and no metric other than :func:`token_accuracy` closures of the loss's own
    ``ignore_index`` (``model.loss`` returns that accuracy).  Anything else runs the loop on the logits."""
    return (isinstance(loss_fn, ResidueTaskLoss) and callable(getattr(model, "loss", None))
            and all(getattr(m, "token_accuracy_ignore_index", None) == loss_fn.ignore_index
                    for m in metrics.values()))


def test_step(model: torch.nn.Module, dataloader, loss_fn: torch.nn.Module, metrics: Dict[str, Callable],
              device=None, distributed: bool = False, collect: Optional[list] = None
              ) -> Tuple[float, Dict[str, float]]:
    """``collect``: a list that receives every batch's ``(outputs, y)`` (for metrics that are not batch means,
    e.g. :func:`spearman` over the whole test set)."""
    device = torch.device(device or _default_device())
    model.eval()
    loss_sum = torch.zeros((), dtype=torch.float32, device=device)
    met_sum = {k: torch.zeros((), dtype=torch.float32, device=device) for k in metrics}
    n = 0
    with torch.inference_mode():
        for X, y in dataloader:
            X, y = _to(X, device), _to(y, device)
            logits = model(X)
            loss_sum += loss_fn(logits, y).float()
            preds = torch.softmax(logits.float(), dim=1)
            for k, m in metrics.items():
                met_sum[k] += _metric_value(m(preds, y)).to(device)
            if collect is not None:
                collect.append((logits.float(), y))
            n += 1
    return _finish(loss_sum, met_sum, n, distributed)


def _finish(loss_sum, met_sum, n, distributed, counter=None) -> Tuple[float, Dict[str, float]]:
    """The epoch's one host read.  ``counter`` (``ResidueTaskLoss.counter``) travels in the same copy; labels
    it counted as ``>= n_classes`` are an error."""
    vals = torch.stack([loss_sum] + [met_sum[k] for k in met_sum]) / max(1, n)
    if distributed:
        pdist.all_reduce_mean_(vals)
    if counter is not None:
        host = torch.cat([vals.double(), counter[N_BAD:N_BAD + 1].double()]).cpu().tolist()
        vals, bad = host[:-1], int(host[-1])
        if bad:
            raise ValueError(f"{bad} training labels are outside the head's classes; labels below 0 are ignored")
    else:
        vals = vals.cpu().tolist()
    return vals[0], {k: v for k, v in zip(met_sum, vals[1:])}


# ---- metrics for per-residue tasks (ignore_index-aware) ----------------------------------------
def token_accuracy(ignore_index: int = -100) -> Callable:
    """Accuracy over non-ignored residues; ``preds`` ``[B, K, L]`` probabilities, ``y`` ``[B, L]``."""
    def _acc(preds: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        valid = y != ignore_index
        hit = (preds.argmax(1) == y) & valid
        return hit.sum().float() / valid.sum().clamp_min(1).float()
    _acc.token_accuracy_ignore_index = ignore_index      # train_step recognises the closure by this tag
    return _acc


def sequence_accuracy() -> Callable:
    """Accuracy of a per-protein classifier; ``preds`` ``[B, K]`` probabilities, ``y`` ``[B]``."""
    def _acc(preds: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return (preds.argmax(1) == y).float().mean()
    return _acc


def regression_loss() -> Callable:
    """MSE between the ``[B, 1]`` output of an ``n_classes=1`` head and the float targets ``[B]``."""
    def _mse(out: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return F.mse_loss(out.float().reshape(-1), y.float().reshape(-1))
    return _mse


def _average_ranks(v: torch.Tensor) -> torch.Tensor:
    """1-based ranks of a 1-D tensor, tied values sharing the mean of the ranks they span (fp64)."""
    v = v.reshape(-1)
    order = torch.argsort(v, stable=True)
    sv = v[order]
    n = v.numel()
    first = torch.ones(n, dtype=torch.bool, device=v.device)
    first[1:] = sv[1:] != sv[:-1]
    grp = torch.cumsum(first.long(), 0) - 1                       # tie group of every sorted element
    pos = torch.arange(1, n + 1, dtype=torch.float64, device=v.device)
    ng = int(grp[-1].item()) + 1 if n else 0
    sums = torch.zeros(ng, dtype=torch.float64, device=v.device).index_add_(0, grp, pos)
    cnt = torch.zeros(ng, dtype=torch.float64, device=v.device).index_add_(0, grp, torch.ones_like(pos))
    ranks = torch.empty(n, dtype=torch.float64, device=v.device)
    ranks[order] = (sums / cnt)[grp]
    return ranks


def spearman(pred: torch.Tensor, y: torch.Tensor) -> float:
    """Spearman rank correlation of two equally long value sets: the Pearson correlation of their ranks, ties
    given average ranks.  0.0 when either side is constant (the correlation is undefined there)."""
    p, t = pred.detach().reshape(-1).double(), y.detach().reshape(-1).double()
    if p.numel() != t.numel():
        raise ValueError(f"spearman: {p.numel()} predictions for {t.numel()} targets")
    if p.numel() < 2:
        return 0.0
    rp, rt = _average_ranks(p), _average_ranks(t)
    rp, rt = rp - rp.mean(), rt - rt.mean()
    den = torch.sqrt((rp * rp).sum() * (rt * rt).sum())
    return float((rp * rt).sum() / den) if den > 0 else 0.0


EVALUATE_MODES = ("batch_mean", "exact")
SMALLER_IS_BETTER = ("loss", "mse", "mae")


def finetune(model: torch.nn.Module, train_dataloader, optimizer: torch.optim.Optimizer, epochs: int = 1,
             test_dataloader=None, loss_fn: Optional[torch.nn.Module] = None, metrics: Optional[Dict] = None,
             gradient_clipping: bool = True, gradient_clipping_thresh: float = 1.0, device=None,
             ddp=None, log: Optional[Callable[[str], None]] = None,
             epoch_metrics: Optional[Dict[str, Callable]] = None, evaluate: str = "batch_mean",
             select_metric: Optional[str] = None, patience: Optional[int] = None) -> Dict[str, Any]:
    """Epoch loop around :func:`train_step` / :func:`test_step` (the shape of the reference's
    commented ``train()``, ``utils.py:348-460``).

    ``epoch_metrics``: ``name -> fn(outputs, y)`` evaluated once per epoch on the model's raw outputs over the
    whole test set (this rank's share of it), e.g. ``{"spearman": spearman}``: such a statistic is not a mean
    of per-batch values.  Reported in ``results["test_metrics"]`` beside the batch-mean metrics.

    ``evaluate``: ``"batch_mean"`` (the default) is :func:`test_step`, the reference's mean of per-batch values.
    ``"exact"`` (needs ``test_dataloader``) runs :func:`.evaluate_finetune.evaluate_finetune` per epoch instead:
    whole-set sums, the confusion matrix and what follows from it.  ``results["test_eval"]`` gets the metric
    dicts, ``results["test_loss"]`` their ``loss`` (``mse`` for regression) and ``results["test_metrics"]`` their
    scalars.  Under ``ddp`` a test loader whose sampler is a :class:`..parallel.sampler.ShardedSampler` is this
    rank's shard and the sums are all-reduced; any other test loader is evaluated whole by every rank.

    ``select_metric`` (needs ``evaluate="exact"``): a scalar of those dicts; larger is better except for
    ``loss``, ``mse`` and ``mae``, and ``nan`` never wins.  The trainable parameters of the best epoch are kept
    as a CPU copy and loaded back after the last epoch; ``results["best_epoch"]`` (0-based) and
    ``results["best_metric"]`` name it.  ``patience=p`` (needs ``select_metric``): stop after ``p`` epochs
    without improvement; ``results["stopped_early"]`` records whether that happened."""
    loss_fn = loss_fn or torch.nn.CrossEntropyLoss(ignore_index=-100)
    metrics = metrics if metrics is not None else {"accuracy": token_accuracy()}
    results: Dict[str, Any] = {"train_loss": [], "test_loss": [], "train_metrics": [], "test_metrics": []}
    if evaluate not in EVALUATE_MODES:
        raise ValueError(f"evaluate={evaluate!r}: expected one of {EVALUATE_MODES}")
    exact = evaluate == "exact"
    if exact and test_dataloader is None:
        raise ValueError('evaluate="exact" needs a test_dataloader')
    if select_metric is not None and not exact:
        raise ValueError('select_metric needs evaluate="exact"')
    if patience is not None and (select_metric is None or patience < 1):
        raise ValueError("patience needs select_metric and a value >= 1")
    if exact:
        from .evaluate_finetune import evaluate_finetune, scalar_metrics
        from ..parallel.sampler import ShardedSampler
        sharded = ddp is not None and isinstance(getattr(test_dataloader, "sampler", None), ShardedSampler)
        results["test_eval"] = []
        if select_metric is not None:
            results.update(best_epoch=None, best_metric=None, stopped_early=False)
    best_state: Optional[Dict[str, torch.Tensor]] = None
    for epoch in range(epochs):
        if hasattr(getattr(train_dataloader, "sampler", None), "set_epoch"):
            train_dataloader.sampler.set_epoch(epoch)
        tl, tm = train_step(model, train_dataloader, loss_fn, optimizer, metrics, gradient_clipping,
                            gradient_clipping_thresh, device, ddp)
        results["train_loss"].append(tl)
        results["train_metrics"].append(tm)
        if exact:
            m = evaluate_finetune(model, test_dataloader, device=device, distributed=sharded)
            results["test_eval"].append(m)
            results["test_loss"].append(m["loss"] if "loss" in m else m["mse"])
            results["test_metrics"].append(scalar_metrics(m))
        elif test_dataloader is not None:
            seen: Optional[list] = [] if epoch_metrics else None
            vl, vm = test_step(model, test_dataloader, loss_fn, metrics, device, ddp is not None, collect=seen)
            if seen:
                out_all, y_all = torch.cat([o for o, _ in seen]), torch.cat([t for _, t in seen])
                for k, m in epoch_metrics.items():
                    vm[k] = float(m(out_all, y_all))
            results["test_loss"].append(vl)
            results["test_metrics"].append(vm)
        if log is not None and pdist.is_main():
            log(f"epoch {epoch + 1}/{epochs} train_loss={tl:.4f} {tm} "
                + (f"test_loss={results['test_loss'][-1]:.4f} {results['test_metrics'][-1]}"
                   if test_dataloader is not None else ""))
        if select_metric is not None:
            if select_metric not in results["test_metrics"][-1]:
                raise ValueError(f"select_metric={select_metric!r}: the evaluation's scalars are "
                                 f"{sorted(results['test_metrics'][-1])}")
            v = float(results["test_metrics"][-1][select_metric])
            best = results["best_metric"]
            if v == v and (best is None or (v < best if select_metric in SMALLER_IS_BETTER else v > best)):
                results.update(best_epoch=epoch, best_metric=v)
                best_state = {k: p.detach().to("cpu", copy=True) for k, p in model.named_parameters()
                              if p.requires_grad}
            elif patience is not None and epoch - (-1 if results["best_epoch"] is None
                                                   else results["best_epoch"]) >= patience:
                results["stopped_early"] = True
                break
    if best_state is not None and results["best_epoch"] != len(results["train_loss"]) - 1:
        with torch.no_grad():
            for k, p in model.named_parameters():
                if k in best_state:
                    p.copy_(best_state[k])
    return results


test_step.__test__ = False   # reference name; not a pytest test when imported into test modules
