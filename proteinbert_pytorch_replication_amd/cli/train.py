"""Training CLIs: ``pretrain`` and ``finetune`` (config presets + ``section.key=value`` overrides).

    python -m proteinbert_pytorch_replication_amd.cli pretrain --preset cfg2_paper_l512 \\
        train.max_batch_iterations=1000 data.source=store data.path=/data/uniref90.pbxds
    torchrun --nproc-per-node 8 -m proteinbert_pytorch_replication_amd.cli pretrain --preset ...

``data.source``: ``synthetic`` (on-device UniRef90-shaped batches), ``store`` (a ``.pbxds``/``.h5``
store or a directory of them, read by the native loader) or ``dataframe`` (``data.path`` = a CSV
with ``seq`` and space-separated ``annotations`` index columns).  The reference's own driver is
``dummy_tests.py`` (see :mod:`.dummy_tests`).

``finetune``: frozen (or full) encoder + a task head, on synthetic data or CSVs.  ``--task residue`` (the
default): per-residue classes, CSV columns ``seq`` and ``labels`` (one class character per residue, classes
given by ``--classes``).  ``--task sequence``: per-protein classes, columns ``seq`` and ``label`` (an integer in
``0..n-1``, ``--n-classes n``), accuracy.  ``--task regression``: columns ``seq`` and ``label`` (a float), MSE
loss and the test set's Spearman correlation per epoch.  ``--hidden all`` puts the head on every block's hidden
state instead of the last block's (:mod:`..models.finetune`).  The head is saved as
``proteinbert_finetuned_head.pt`` (``"head"`` in the printed JSON); ``--unfreeze`` also saves the encoder it
trained as a model file (``"encoder"``), the pair ``cli predict --model ... --head NAME=...`` takes.
``--eval exact`` evaluates the test set per epoch with whole-set sums, the confusion matrix and per-class metrics
(:mod:`..train.evaluate_finetune`) instead of the mean of per-batch values; ``--select-metric NAME`` then saves
the head of the epoch that is best by that scalar and ``--patience N`` stops after N epochs without improvement
(``"test_eval"`` and ``"best_epoch"`` in the printed JSON).  ``cli evaluate`` (:mod:`.evaluate`) reports the same
metrics for a saved head.
``--task residue`` can shape its training loss (:mod:`..train.task_loss`): ``--class-weights balanced`` (from one
pass over the training labels) or ``--class-weights w0,w1,...`` (one weight per class), ``--label-smoothing E``;
``--fused-loss`` selects the same loss object with neither, i.e. the plain cross-entropy on the fused
loss launch.  ``"loss"`` in the printed JSON records the weights and the smoothing used.
"""
from __future__ import annotations

import argparse
import json
import logging
import os
from typing import List, Optional

import torch

from ..config import RunConfig, apply_overrides, get_preset, load_yaml, PRESETS
from ..data import SyntheticUniRefGO, CorruptionParams
from ..models import (ProteinBERT, ProteinBERTForSequenceClassification, ProteinBERTForTokenClassification,
                      build_model)
from ..models.finetune import build_finetune_model, load_finetuned_head  # noqa: F401  (their home; names kept here)
from ..utils import determinism
from ..parallel import dist as pdist


def _cfg(args) -> RunConfig:
    cfg = load_yaml(args.config) if args.config else get_preset(args.preset)
    return apply_overrides(cfg, args.overrides)


def _common(p: argparse.ArgumentParser) -> None:
    p.add_argument("--preset", default="cfg2_paper_l512", choices=sorted(PRESETS))
    p.add_argument("--config", default=None, help="YAML config (optionally with a `preset:` key)")
    p.add_argument("overrides", nargs="*", help="section.key=value overrides")


class _DataFrameAnnotations:
    """CSV -> reference DataFrame dataset rows (sequence, dense 0/1 annotation list)."""

    @staticmethod
    def load(path: str, num_annotations: int):
        import pandas as pd
        df = pd.read_csv(path)
        rows = []
        for seq, ann in zip(df["seq"], df.get("annotations", [""] * len(df))):
            dense = [0] * num_annotations
            for tok in str(ann).split():
                if tok and tok != "nan":
                    dense[int(tok)] = 1
            rows.append((seq, dense))
        return pd.DataFrame(rows)


def pretrain_main(argv: Optional[List[str]] = None) -> dict:
    ap = argparse.ArgumentParser(description="ProteinBERT pretraining (MI355X)")
    _common(ap)
    ap.add_argument("--resume", choices=["none", "latest"], default="latest")
    ap.add_argument("--metrics", default=None, help="JSONL metrics file (rank 0)")
    ap.add_argument("--tensorboard", default=None, help="TensorBoard event-file directory (rank 0)")
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--async-checkpoint", action="store_true")
    ap.add_argument("--profile-steps", default=None, help="START[:COUNT] steps traced with torch.profiler")
    ap.add_argument("--profile-dir", default=None, help="trace output directory (default: save path)")
    ap.add_argument("--zero", action="store_true", help="ZeRO-1: shard the Adam moments over the DP ranks")
    a = ap.parse_args(argv)
    cfg = _cfg(a)
    logging.basicConfig(format="%(asctime)s [%(levelname)s]: %(message)s", level=logging.INFO)
    info = pdist.init_distributed(backend=cfg.dist.backend, timeout_s=cfg.dist.timeout_s)
    dev = info.device
    if cfg.kernel.deterministic:
        determinism.enable()
    if cfg.kernel.gelu != "fitted":
        from ..ops import _lib as _hiplib
        _hiplib.set_gelu(cfg.kernel.gelu)
    torch.manual_seed(cfg.train.seed)
    if cfg.data.lengths:
        # multi-length schedule: the LayerNorm affine is stored at the longest L and sliced per batch
        import dataclasses
        cfg.model = dataclasses.replace(cfg.model, sequences_length=max(int(x) for x in cfg.data.lengths),
                                        variable_length=True)
    model = build_model(cfg.model, device=dev, backend=determinism.backend_for(cfg.kernel.backend, cfg.model))
    B, L = cfg.train.batch_size, cfg.model.sequences_length
    corr = CorruptionParams(cfg.data.token_corruption_p, cfg.data.annotation_positive_p,
                            cfg.data.annotation_negative_p, cfg.data.blank_annotation_p)

    def make_loader(path, seed):
        if cfg.data.source == "synthetic" and cfg.data.lengths:
            from ..data.synthetic import MultiLengthSynthetic
            return MultiLengthSynthetic(cfg.data.lengths, cfg.model.num_annotations, B, dev,
                                        seed=seed + 1000 * info.rank, min_length=cfg.data.min_length,
                                        density=cfg.data.annotation_density, corruption=corr)
        if cfg.data.source == "synthetic":
            return SyntheticUniRefGO(L, cfg.model.num_annotations, B, dev, min_length=cfg.data.min_length,
                                     max_length=cfg.data.max_length, density=cfg.data.annotation_density,
                                     seed=seed + 1000 * info.rank, corruption=corr)
        if cfg.data.source in ("store", "hdf5"):
            from ..train.dataloaders import create_pretrain_dataloaders
            return create_pretrain_dataloaders(path, B, recursive_dir=True, num_workers=cfg.data.num_workers,
                                               seq_max_length=L, device=dev, seed=seed)
        if cfg.data.source == "dataframe":
            from torch.utils.data import DataLoader
            from ..data import UniRefGO_PretrainingDataset, collate_triples
            from ..parallel.sampler import ShardedSampler
            ds = UniRefGO_PretrainingDataset(_DataFrameAnnotations.load(path, cfg.model.num_annotations),
                                             seq_max_length=L)
            return DataLoader(ds, batch_size=B, sampler=ShardedSampler(len(ds), info.rank, info.world_size),
                              num_workers=cfg.data.num_workers, collate_fn=collate_triples, drop_last=True)
        raise ValueError(f"unknown data.source {cfg.data.source!r}")

    loader = make_loader(cfg.data.path, cfg.data.seed)
    # held-out evaluation (eval.every > 0): the same source read from eval.path; the synthetic source gets a
    # second generator of its own seed (endless: eval.batches bounds it, 8 by default)
    eval_loader, eval_batches = None, cfg.eval.batches
    if cfg.eval.every > 0:
        if cfg.data.source == "synthetic":
            eval_loader = make_loader(None, cfg.eval.seed)
            eval_batches = 8 if eval_batches is None else eval_batches
        elif cfg.eval.path is None:
            raise ValueError("eval.every > 0 needs eval.path (the held-out data) for data.source "
                             f"{cfg.data.source!r}")
        else:
            eval_loader = make_loader(cfg.eval.path, cfg.data.seed)
    if cfg.optim.decoupled_weight_decay or (cfg.optim.no_decay_norm_bias and cfg.optim.weight_decay):
        # AdamW and / or weight decay that skips biases and LayerNorm affines: parameter groups, which
        # pretrain() turns into one FusedAdam over the model's arena
        from ..train.optim import param_groups_for
        groups = param_groups_for(model, cfg.optim.lr, cfg.optim.weight_decay,
                                  no_decay=("bias", "norm") if cfg.optim.no_decay_norm_bias else ())
        cls = torch.optim.AdamW if cfg.optim.decoupled_weight_decay else torch.optim.Adam
        opt = cls(groups, lr=cfg.optim.lr, betas=cfg.optim.betas, eps=cfg.optim.eps,
                  weight_decay=cfg.optim.weight_decay)
    else:
        opt = torch.optim.Adam(model.parameters(), lr=cfg.optim.lr, betas=cfg.optim.betas, eps=cfg.optim.eps,
                               weight_decay=cfg.optim.weight_decay)
    from ..train.pretrain import pretrain
    res = pretrain(model, loader, opt, max_batch_iterations=cfg.train.max_batch_iterations,
                   save_path=cfg.train.save_path, nb_iterations_checkpoint=cfg.train.nb_iterations_checkpoint,
                   optim_scheduler_patience=cfg.optim.plateau_patience, warmup_duration=cfg.optim.warmup_duration,
                   device=dev, log_every=a.log_every, bucket_mb=cfg.dist.bucket_mb, compute_dtype=cfg.kernel.dtype,
                   grad_clip=cfg.optim.grad_clip, async_checkpoint=a.async_checkpoint, metrics_path=a.metrics,
                   tensorboard_dir=a.tensorboard,
                   resume=a.resume, profile_steps=a.profile_steps, profile_dir=a.profile_dir,
                   zero_optimizer=a.zero, comm_dtype=cfg.dist.comm_dtype,
                   dp_batch_softmax=cfg.dist.dp_batch_softmax, eval_dataloader=eval_loader,
                   eval_every=cfg.eval.every, eval_batches=eval_batches)
    if info.is_main:
        out = {"final_loss": res["train_loss"][-1] if res["train_loss"] else None,
               "iterations": len(res["train_loss"]), "final_model": res.get("final_model_path")}
        if res.get("eval"):
            from ..train.evaluate import scalar_metrics
            out["eval"] = scalar_metrics(res["eval"][-1])
        print(json.dumps(out))
    return res


def _ss_csv(path: str, L: int, classes: str):
    import pandas as pd
    from ..data.vocab import create_amino_acid_vocab, SOS_ID, EOS_ID
    v = create_amino_acid_vocab()
    cmap = {c: i for i, c in enumerate(classes)}
    df = pd.read_csv(path)
    toks, labs = [], []
    for seq, lab in zip(df["seq"], df["labels"]):
        seq, lab = str(seq)[: L - 2], str(lab)[: L - 2]
        t = [SOS_ID] + list(v.encode(seq)) + [EOS_ID]
        y = [-100] + [cmap.get(c, -100) for c in lab] + [-100]
        toks.append(t + [0] * (L - len(t)))
        labs.append(y + [-100] * (L - len(y)))
    return torch.utils.data.TensorDataset(torch.tensor(toks), torch.tensor(labs))


def _seq_csv(path: str, L: int, regression: bool, n_classes: int):
    """``seq,label`` CSV -> (tokens [N, L], labels [N]): float targets (regression) or classes ``0..n-1``."""
    import pandas as pd
    from ..data.vocab import create_amino_acid_vocab, SOS_ID, EOS_ID
    v = create_amino_acid_vocab()
    df = pd.read_csv(path)
    toks = []
    for seq in df["seq"]:
        t = [SOS_ID] + list(v.encode(str(seq)[: L - 2])) + [EOS_ID]
        toks.append(t + [0] * (L - len(t)))
    if regression:
        labs = torch.tensor([float(x) for x in df["label"]], dtype=torch.float32)
    else:
        labs = torch.tensor([int(x) for x in df["label"]], dtype=torch.int64)
        if len(labs) and (int(labs.min()) < 0 or int(labs.max()) >= n_classes):
            raise ValueError(f"{path}: labels must lie in 0..{n_classes - 1} (--n-classes {n_classes})")
    return torch.utils.data.TensorDataset(torch.tensor(toks), labs)


FINETUNE_TASKS = ("residue", "sequence", "regression")


def finetune_main(argv: Optional[List[str]] = None) -> dict:
    ap = argparse.ArgumentParser(description="ProteinBERT fine-tuning: per-residue / per-protein task heads")
    _common(ap)
    ap.add_argument("--pretrained", default=None, help="pretrained model/checkpoint (.pt) to start from")
    ap.add_argument("--train-csv", default=None)
    ap.add_argument("--test-csv", default=None)
    ap.add_argument("--classes", default="HEC", help="label alphabet (e.g. HEC or DSSP8 'HGIEBTSC')")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--unfreeze", action="store_true", help="train the encoder as well")
    ap.add_argument("--encoder-lr", type=float, default=None,
                    help="with --unfreeze: the encoder's learning rate (default: --lr, one parameter group)")
    ap.add_argument("--weight-decay", type=float, default=0.0,
                    help="weight decay on everything but biases and LayerNorm affines")
    ap.add_argument("--decoupled", action="store_true", help="AdamW (decoupled weight decay) instead of Adam")
    ap.add_argument("--synthetic-samples", type=int, default=2048)
    ap.add_argument("--task", default="residue", choices=FINETUNE_TASKS,
                    help="residue: per-residue classes; sequence: per-protein classes; regression: per-protein value")
    ap.add_argument("--hidden", default="last", choices=("last", "all"),
                    help="head input: the last block's hidden state, or every block's, concatenated")
    ap.add_argument("--n-classes", type=int, default=2, help="--task sequence: number of classes")
    ap.add_argument("--eval", default="batch-mean", choices=("batch-mean", "exact"), dest="eval_mode",
                    help="test-set evaluation per epoch: the mean of per-batch values, or exact whole-set sums "
                         "with the confusion matrix and per-class metrics")
    ap.add_argument("--select-metric", default=None,
                    help="with --eval exact: keep the epoch that is best by this scalar (e.g. macro_f1, loss)")
    ap.add_argument("--patience", type=int, default=None,
                    help="with --select-metric: stop after this many epochs without improvement")
    ap.add_argument("--class-weights", default=None,
                    help="--task residue: 'balanced' (n_live / (n_classes * count_k) over the training labels) or "
                         "one weight per class, comma-separated")
    ap.add_argument("--label-smoothing", type=float, default=None, help="--task residue: 0 <= E < 1")
    ap.add_argument("--fused-loss", action="store_true",
                    help="--task residue: the plain cross-entropy through the fused loss launch")
    a = ap.parse_args(argv)
    cfg = _cfg(a)
    logging.basicConfig(format="%(asctime)s [%(levelname)s]: %(message)s", level=logging.INFO)
    info = pdist.init_distributed(backend=cfg.dist.backend)
    if a.task == "sequence" and a.n_classes < 2:
        raise ValueError("--task sequence needs --n-classes >= 2")
    shaped = a.class_weights is not None or a.label_smoothing is not None or a.fused_loss
    if shaped and a.task != "residue":
        raise ValueError("--class-weights / --label-smoothing / --fused-loss need --task residue")
    if a.label_smoothing is not None and not 0.0 <= a.label_smoothing < 1.0:
        raise ValueError(f"--label-smoothing {a.label_smoothing}: expected 0 <= E < 1")
    class_weights = None
    if a.class_weights is not None and a.class_weights != "balanced":
        try:
            class_weights = [float(v) for v in a.class_weights.split(",")]
        except ValueError:
            raise ValueError(f"--class-weights {a.class_weights!r}: expected 'balanced' or w0,w1,...") from None
        if len(class_weights) != len(a.classes):
            raise ValueError(f"--class-weights has {len(class_weights)} weights for the {len(a.classes)} classes "
                             f"of --classes {a.classes!r}")
    if cfg.kernel.deterministic:
        determinism.enable()
    if cfg.kernel.gelu != "fitted":
        from ..ops import _lib as _hiplib
        _hiplib.set_gelu(cfg.kernel.gelu)
    dev = info.device
    torch.manual_seed(cfg.train.seed)
    if a.pretrained:
        from ..train.checkpoint import load_model
        enc = load_model(a.pretrained, device=dev, backend=determinism.backend_for(cfg.kernel.backend, cfg.model))
    else:
        enc = build_model(cfg.model, device=dev, backend=determinism.backend_for(cfg.kernel.backend, cfg.model))
    L = enc.config["sequences_length"]
    n_classes = {"residue": len(a.classes), "sequence": a.n_classes, "regression": 1}[a.task]
    meta = {"task": a.task, "hidden": a.hidden, "n_classes": n_classes,
            "classes": a.classes if a.task == "residue" else None, "use_global": a.task == "residue"}
    model = build_finetune_model(enc, meta, freeze_encoder=not a.unfreeze)
    from torch.utils.data import DataLoader
    from ..data.synthetic import SyntheticSecondaryStructure, SyntheticSequenceTask
    from ..parallel.sampler import ShardedSampler
    if a.task != "residue":
        if a.train_csv:
            train_ds = _seq_csv(a.train_csv, L, a.task == "regression", n_classes)
            test_ds = _seq_csv(a.test_csv, L, a.task == "regression", n_classes) if a.test_csv else None
        else:
            train_ds = SyntheticSequenceTask(a.synthetic_samples, L, n_classes, seed=cfg.train.seed)
            test_ds = SyntheticSequenceTask(max(64, a.synthetic_samples // 8), L, n_classes, seed=cfg.train.seed + 1)
    elif a.train_csv:
        train_ds = _ss_csv(a.train_csv, L, a.classes)
        test_ds = _ss_csv(a.test_csv, L, a.classes) if a.test_csv else None
    else:
        train_ds = SyntheticSecondaryStructure(a.synthetic_samples, L, len(a.classes), seed=cfg.train.seed)
        test_ds = SyntheticSecondaryStructure(max(64, a.synthetic_samples // 8), L, len(a.classes),
                                              seed=cfg.train.seed + 1)
    B = cfg.train.batch_size
    dl = DataLoader(train_ds, batch_size=B, sampler=ShardedSampler(len(train_ds), info.rank, info.world_size),
                    drop_last=True)
    tl = DataLoader(test_ds, batch_size=B) if test_ds is not None else None
    from ..train.optim import FusedAdam, make_optimizer, param_groups_for
    enc_lr = a.lr if a.encoder_lr is None else a.encoder_lr
    if a.unfreeze and enc_lr != a.lr:
        # the pretrained encoder and the fresh head as two (with weight decay: up to four) groups of one FusedAdam
        if a.lr == 0:
            raise ValueError("--encoder-lr needs a non-zero --lr (it is applied as a factor on it)")
        groups = param_groups_for(model, a.lr, a.weight_decay, lr_scale={"encoder.": enc_lr / a.lr})
        for g in groups:
            if g["lr"] != a.lr:
                g["lr"] = enc_lr            # the rate as given, not lr * (encoder_lr / lr)
        opt = make_optimizer(model, lr=a.lr, weight_decay=a.weight_decay, groups=groups,
                             decoupled_weight_decay=a.decoupled)
    elif a.weight_decay or a.decoupled:
        opt = make_optimizer(model, lr=a.lr, weight_decay=a.weight_decay, groups=param_groups_for(
            model, a.lr, a.weight_decay), decoupled_weight_decay=a.decoupled)
    else:
        params = [p for p in model.parameters() if p.requires_grad]
        opt = FusedAdam(params, lr=a.lr)
    ddp = None
    if info.distributed:
        from ..parallel.ddp import BucketedAllReduce
        ddp = BucketedAllReduce(opt.arena, bucket_mb=cfg.dist.bucket_mb)
        ddp.broadcast_parameters(model)
        opt.grad_scale = 1.0 / info.world_size
    from ..train.finetune import finetune, regression_loss, sequence_accuracy, spearman, token_accuracy
    loss_info = None
    if a.task == "residue":
        task_args = dict(metrics={"accuracy": token_accuracy()})
        if shaped:
            from ..train.task_loss import ResidueTaskLoss, balanced_class_weights
            if a.class_weights == "balanced":
                # one pass over this rank's view of the training set's labels (every rank holds the whole set)
                labels = train_ds.tensors[1] if a.train_csv else train_ds.labels
                class_weights = balanced_class_weights(labels, n_classes).tolist()
            task_args["loss_fn"] = ResidueTaskLoss(class_weights, a.label_smoothing or 0.0)
            if class_weights is not None or a.label_smoothing is not None:
                loss_info = {"class_weights": class_weights, "label_smoothing": a.label_smoothing or 0.0}
    elif a.task == "sequence":
        task_args = dict(metrics={"accuracy": sequence_accuracy()}, loss_fn=torch.nn.CrossEntropyLoss())
    else:
        # Spearman is a statistic of the whole test set, computed once per epoch, not a mean over batches
        task_args = dict(metrics={}, loss_fn=regression_loss(), epoch_metrics={"spearman": spearman})
    if a.eval_mode == "exact":
        # the selected epoch's parameters are back in the model when finetune returns: the files below hold them
        task_args.update(evaluate="exact", select_metric=a.select_metric, patience=a.patience)
    elif a.select_metric is not None or a.patience is not None:
        raise ValueError("--select-metric / --patience need --eval exact")
    res = finetune(model, dl, opt, epochs=a.epochs, test_dataloader=tl, device=dev, ddp=ddp, log=print, **task_args)
    res["optimizer"] = opt
    res["meta"] = meta
    res["model"] = model
    if info.is_main:
        os.makedirs(cfg.train.save_path, exist_ok=True)
        path = os.path.join(cfg.train.save_path, "proteinbert_finetuned_head.pt")
        head = {k: v for k, v in model.state_dict().items() if not k.startswith("encoder.")}
        # the default form keeps the file it always had (tensors only), which load_finetuned_head reads as
        # task="residue", hidden="last"; every other form says what it is
        if (a.task, a.hidden) != ("residue", "last"):
            head["meta"] = meta
        torch.save(head, path)
        res["head"] = path
        summary = {"train_loss": res["train_loss"], "test_metrics": res["test_metrics"], "head": path}
        if a.eval_mode == "exact":
            summary["test_eval"] = res["test_metrics"][-1] if res["test_metrics"] else None
            summary["best_epoch"] = res.get("best_epoch")
        if loss_info is not None:
            summary["loss"] = loss_info
        if a.unfreeze:
            # the head file holds no encoder entries: without the encoder it was trained with, the head could
            # never be used (inference.Predictor(load_model(encoder), heads={...: head file}))
            from ..train.checkpoint import save_final_model
            res["encoder"] = summary["encoder"] = save_final_model(model.encoder, cfg.train.save_path)
        print(json.dumps(summary))
    return res
