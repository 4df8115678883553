#!/usr/bin/env python3
"""Linear evaluation of an upstream checkpoint on the MI355X path (the DINO / MSN / BYOL-A protocol): the train, validation and test
CSVs are embedded ONCE with the frozen encoder, the features are standardised with the training statistics, a whole grid of linear
heads - one per (learning rate, weight decay) pair - is trained together on the cached matrix, the head is picked on the validation
split and its test accuracy is reported.

    python audio-ssl_amd/evaluate_linear.py --checkpoint final.ckpt --upstream delores_m --train_csv train.csv --test_csv test.csv

The CSVs are `train_downstream.py`'s (`wav,label`); label ids are sorted as `DownstreamDataset` sorts them.  Without `--valid_csv`
a stratified hold-out of the training rows (`--holdout`, `--seed`) is the validation split.  `--embeddings DIR` reads what
`--dump_embeddings DIR` of this command or of `evaluate_knn.py` wrote instead of embedding again.  Prints one JSON line:
{"top1", "lr", "wd", "val_top1", "heads", "N_train", "N_valid", "N_test", "d", "epochs"}.  Single GPU and single-label: multi-label
tasks stay with `train_tagging.py`, and training over several ranks is out of scope.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

DEFAULT_LRS = "1e-4,3e-4,1e-3,3e-3,1e-2,3e-2"
DEFAULT_WDS = "0,1e-4,1e-2"


def float_list(text):
    vals = [float(v) for v in str(text).split(",") if v.strip()]
    if not vals or any(v < 0 for v in vals):
        raise argparse.ArgumentTypeError(f"expected a comma list of non-negative numbers, got {text!r}")
    return vals


def _embed(args):
    """-> (train, y_train, valid | None, y_valid | None, test, y_test, label names): fp32 device matrices, int64 CPU labels."""
    import pandas as pd
    import yaml
    from src.evaluation import extract_embeddings, load_embedder
    config = None
    if args.config:
        with open(args.config, "r") as f:
            config = yaml.load(f, Loader=yaml.SafeLoader)
    frames = [pd.read_csv(args.train_csv), pd.read_csv(args.valid_csv) if args.valid_csv else None, pd.read_csv(args.test_csv)]
    label2id = {k: i for i, k in enumerate(sorted(set(frames[0]["label"]), key=str))}       # DownstreamDataset.get_label2id
    for name, fr in zip((args.train_csv, args.valid_csv, args.test_csv), frames):
        if fr is not None:
            unknown = sorted(set(fr["label"]) - set(label2id), key=str)
            if unknown:
                raise ValueError(f"labels of {name} that {args.train_csv} does not have: {unknown[:5]}")
    embedder = load_embedder(args.checkpoint, args.upstream, config=config, layer=args.layer)
    duration = float(embedder.model.config["pretrain"]["input"]["length_wave"])
    kw = dict(batch_size=args.batch_size, window=args.window, duration=duration, max_duration=args.max_duration)
    out = []
    for fr in frames:
        if fr is None:
            out += [None, None]
        else:
            out += [extract_embeddings(embedder, list(fr["wav"]), **kw),
                    torch.tensor([label2id[v] for v in fr["label"]], dtype=torch.int64)]
    return (*out, [str(k) for k in label2id])


def _load(args):
    def arr(name, required=True):
        path = os.path.join(args.embeddings, name + ".npy")
        if not os.path.exists(path):
            if required:
                raise FileNotFoundError(path)
            return None
        return np.load(path)
    x_tr, y_tr, x_te, y_te = arr("train_embeddings"), arr("train_labels"), arr("test_embeddings"), arr("test_labels")
    x_va, y_va = arr("valid_embeddings", False), arr("valid_labels", False)
    names = arr("label_names", False)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()     # noqa: E731
    lab = lambda a: None if a is None else torch.from_numpy(a.astype(np.int64))                                   # noqa: E731
    n_cls = int(y_tr.max()) + 1
    names = [str(v) for v in names.tolist()] if names is not None else [str(i) for i in range(n_cls)]
    return dev(x_tr), lab(y_tr), dev(x_va), lab(y_va), dev(x_te), lab(y_te), names


def main(args):
    from src.evaluation import LinearProbeGrid, feature_stats, stratified_holdout
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_linear.py (MI355X path) needs a GPU; the HIP kernels have no CPU fallback")
    x_tr, y_tr, x_va, y_va, x_te, y_te, names = _load(args) if args.embeddings else _embed(args)
    if args.dump_embeddings:
        os.makedirs(args.dump_embeddings, exist_ok=True)
        parts = [("train_embeddings", x_tr), ("train_labels", y_tr), ("test_embeddings", x_te), ("test_labels", y_te)]
        if x_va is not None:
            parts += [("valid_embeddings", x_va), ("valid_labels", y_va)]
        for name, arr in parts:
            np.save(os.path.join(args.dump_embeddings, name + ".npy"), arr.cpu().numpy())
        np.save(os.path.join(args.dump_embeddings, "label_names.npy"), np.array(names))
    if x_va is None:                                    # stratified hold-out of the training rows
        keep, held = stratified_holdout(y_tr, args.holdout, args.seed)
        if held.numel() == 0:
            raise ValueError("the hold-out is empty: every class has a single training row; pass --valid_csv")
        x_va, y_va = x_tr[held.cuda()].contiguous(), y_tr[held]
        x_tr, y_tr = x_tr[keep.cuda()].contiguous(), y_tr[keep]
    n_cls = max(len(names), int(y_tr.max()) + 1)
    y_tr, y_va, y_te = y_tr.cuda(), y_va.cuda(), y_te.cuda()
    grid = LinearProbeGrid(x_tr.shape[1], n_cls, args.lrs, args.wds, stats=feature_stats(x_tr))
    grid.fit(x_tr, y_tr, args.epochs, args.probe_batch, generator=torch.Generator().manual_seed(args.seed))
    val, test = grid.evaluate(x_va, y_va), grid.evaluate(x_te, y_te)
    best = grid.select(val)
    if args.save_head:
        weight, bias = grid.head(best)
        torch.save(dict(weight=weight.cpu(), bias=bias.cpu(), labels=names, lr=val[best]["lr"], wd=val[best]["wd"]), args.save_head)
    result = dict(top1=test[best]["top1"], lr=val[best]["lr"], wd=val[best]["wd"], val_top1=val[best]["top1"],
                  heads=[dict(lr=v["lr"], wd=v["wd"], val_top1=v["top1"], test_top1=t["top1"]) for v, t in zip(val, test)],
                  N_train=int(x_tr.shape[0]), N_valid=int(x_va.shape[0]), N_test=int(x_te.shape[0]), d=int(x_tr.shape[1]),
                  epochs=args.epochs)
    print(json.dumps(result))
    return result


def get_args(argv=None):
    parser = argparse.ArgumentParser(allow_abbrev=False, description="linear evaluation of an upstream checkpoint: a grid of heads on cached embeddings")
    parser.add_argument("--checkpoint", type=str, default=None, help="path to the pre-trained checkpoint (not needed with --embeddings)")
    parser.add_argument("--upstream", type=str, default="delores_m")
    parser.add_argument("--train_csv", type=str, default=None, help="`wav,label` csv: the training split")
    parser.add_argument("--valid_csv", type=str, default=None, help="`wav,label` csv: the split the head is picked on (default: a hold-out of the training rows)")
    parser.add_argument("--test_csv", type=str, default=None, help="`wav,label` csv: the split that is reported")
    parser.add_argument("-c", "--config", metavar="CONFIG_PATH", default=None, help="yaml overriding the checkpoint's config")
    parser.add_argument("--holdout", type=float, default=0.1, help="without --valid_csv: share of every class's training rows held out for validation")
    parser.add_argument("--seed", type=int, default=0, help="seed of the hold-out and of the epoch permutations")
    parser.add_argument("--lrs", type=float_list, default=float_list(DEFAULT_LRS),
                        help=f"comma list of AdamW learning rates (default {DEFAULT_LRS}: common values, not tuned here)")
    parser.add_argument("--wds", type=float_list, default=float_list(DEFAULT_WDS),
                        help=f"comma list of weight decays (default {DEFAULT_WDS}: common values, not tuned here)")
    parser.add_argument("--epochs", type=int, default=100)
    parser.add_argument("--probe_batch", type=int, default=1024, help="rows per training step of the heads")
    parser.add_argument("--layer", choices=("backbone", "head"), default="backbone")
    parser.add_argument("--window", choices=("center", "random", "whole"), default="center",
                        help="whole: every clip at its own length, in ragged batches (conv encoder)")
    parser.add_argument("--max_duration", type=float, default=30.0, help="--window whole: longer clips are centre-cropped to this many seconds")
    parser.add_argument("--batch_size", type=int, default=64, help="clips per embedding batch")
    parser.add_argument("--dump_embeddings", metavar="DIR", default=None, help="write embeddings and labels as .npy")
    parser.add_argument("--embeddings", metavar="DIR", default=None, help="read the .npy files --dump_embeddings wrote instead of embedding again")
    parser.add_argument("--save_head", metavar="PATH", default=None, help="write the selected head: weight, bias (on raw embeddings), labels, lr, wd")
    args = parser.parse_args(argv)
    if args.embeddings is None and not (args.checkpoint and args.train_csv and args.test_csv):
        parser.error("--checkpoint, --train_csv and --test_csv are required unless --embeddings DIR is given")
    if args.epochs < 1 or args.probe_batch < 1:
        parser.error("--epochs and --probe_batch must be positive")
    if not 0.0 < args.holdout < 1.0:
        parser.error("--holdout must be in (0, 1)")
    return args


if __name__ == "__main__":
    main(get_args())
