#!/usr/bin/env python3
"""Low-shot evaluation of an upstream checkpoint on the MI355X path (the 1 / 5 / 10 labels-per-class protocol of the MSN / DINO /
SimCLR evaluations): the train and test CSVs are embedded ONCE with the frozen encoder, one exact nearest-neighbour graph is built
over both, and label spreading (Zhou et al. 2004) carries `shots` randomly drawn training labels per class to every test clip.
Every (shots value, trial) problem is a group of columns of one pass over the graph; nothing is trained.

    python audio-ssl_amd/evaluate_lowshot.py --checkpoint final.ckpt --upstream delores_m --train_csv train.csv --test_csv test.csv
    python audio-ssl_amd/evaluate_lowshot.py --embeddings DIR --shots 1,5,10 --trials 5

The CSVs are `train_downstream.py`'s (`wav,label`); label ids are sorted as `DownstreamDataset` sorts them.  `--embeddings DIR`
reads what `--dump_embeddings DIR` of this command, of `evaluate_linear.py` or of `evaluate_knn.py` wrote instead of embedding
again.  Prints one JSON line: {"shots", "trials", "top1", "top1_std", "unreached", "short_classes", "k", "sigma", "alpha", "iters",
"N_train", "N_test", "d", "columns"}: `top1` is the mean over the trials for every shots value, `unreached` the share of test clips
no seed reached (they count as wrong), `short_classes` the classes with fewer than `shots` training clips.  Transductive: the
test clips are nodes of the graph.  Single GPU.
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


def int_list(text):
    try:
        vals = [int(v) for v in str(text).split(",") if v.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected a comma list of integers, got {text!r}")
    if not vals or min(vals) < 1:
        raise argparse.ArgumentTypeError(f"expected a comma list of positive integers, got {text!r}")
    return vals


def _embed(args):
    """-> (train, y_train, test, y_test): fp32 device matrices, int64 CPU labels."""
    import pandas as pd
    import yaml
    from src.evaluation import extract_embeddings, load_embedder
    config = None
    if args.config:
        with open(args.config, "r") as f:
            config = yaml.load(f, Loader=yaml.SafeLoader)
    train, test = pd.read_csv(args.train_csv), pd.read_csv(args.test_csv)
    label2id = {k: i for i, k in enumerate(sorted(set(train["label"]), key=str))}       # DownstreamDataset.get_label2id
    unknown = sorted(set(test["label"]) - set(label2id), key=str)
    if unknown:
        raise ValueError(f"labels of {args.test_csv} that {args.train_csv} does not have: {unknown[:5]}")
    embedder = load_embedder(args.checkpoint, args.upstream, config=config, layer=args.layer)
    duration = float(embedder.model.config["pretrain"]["input"]["length_wave"])
    kw = dict(batch_size=args.batch_size, window=args.window, duration=duration, max_duration=args.max_duration)
    out = []
    for fr in (train, test):
        out += [extract_embeddings(embedder, list(fr["wav"]), **kw), torch.tensor([label2id[v] for v in fr["label"]], dtype=torch.int64)]
    return out


def _load(args):
    def arr(name):
        path = os.path.join(args.embeddings, name + ".npy")
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        return np.load(path)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()     # noqa: E731
    lab = lambda a: torch.from_numpy(a.astype(np.int64))                                   # noqa: E731
    return dev(arr("train_embeddings")), lab(arr("train_labels")), dev(arr("test_embeddings")), lab(arr("test_labels"))


def main(args):
    from src.evaluation import lowshot_evaluate
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_lowshot.py (MI355X path) needs a GPU; the HIP kernels have no CPU fallback")
    x_tr, y_tr, x_te, y_te = _load(args) if args.embeddings else _embed(args)
    if args.dump_embeddings:
        os.makedirs(args.dump_embeddings, exist_ok=True)
        for name, arr in (("train_embeddings", x_tr), ("train_labels", y_tr), ("test_embeddings", x_te), ("test_labels", y_te)):
            np.save(os.path.join(args.dump_embeddings, name + ".npy"), arr.cpu().numpy())
    result = lowshot_evaluate(x_tr, y_tr, x_te, y_te, shots=args.shots, trials=args.trials, seed=args.seed, k=args.k, sigma=args.sigma,
                              alpha=args.alpha, iters=args.iters)
    print(json.dumps(result))
    return result


def get_args(argv=None):
    parser = argparse.ArgumentParser(allow_abbrev=False, description="low-shot evaluation of an upstream checkpoint: label spreading on the k-NN graph")
    parser.add_argument("--checkpoint", type=str, default=None, help="path to the pre-trained checkpoint (not needed with --embeddings)")
    parser.add_argument("--upstream", type=str, default="delores_m")
    parser.add_argument("--train_csv", type=str, default=None, help="`wav,label` csv: the clips the labelled shots are drawn from")
    parser.add_argument("--test_csv", type=str, default=None, help="`wav,label` csv: the clips that are scored")
    parser.add_argument("-c", "--config", metavar="CONFIG_PATH", default=None, help="yaml overriding the checkpoint's config")
    parser.add_argument("--layer", choices=("backbone", "head"), default="backbone")
    parser.add_argument("--window", choices=("center", "random", "whole"), default="center",
                        help="whole: every clip at its own length, in ragged batches (conv encoder)")
    parser.add_argument("--max_duration", type=float, default=30.0, help="--window whole: longer clips are centre-cropped to this many seconds")
    parser.add_argument("--batch_size", type=int, default=64, help="clips per embedding batch")
    parser.add_argument("--dump_embeddings", metavar="DIR", default=None, help="write embeddings and labels as .npy")
    parser.add_argument("--embeddings", metavar="DIR", default=None, help="read the .npy files --dump_embeddings wrote instead of embedding again")
    parser.add_argument("--shots", type=int_list, default=int_list("1,5,10"), help="comma list: labelled clips per class")
    parser.add_argument("--trials", type=int, default=5, help="random draws of the labelled clips per shots value")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("-k", type=int, default=10, help="nearest neighbours per node of the graph")
    parser.add_argument("--sigma", type=float, default=None, help="bandwidth of the Gaussian kernel (default: root of the median squared neighbour distance)")
    parser.add_argument("--alpha", type=float, default=0.99, help="share of a node's value that comes from its neighbours")
    parser.add_argument("--iters", type=int, default=None, help="rounds (default: until alpha^iters <= 1e-3)")
    args = parser.parse_args(argv)
    if args.embeddings is None and not (args.checkpoint and args.train_csv and args.test_csv):
        parser.error("--checkpoint, --train_csv and --test_csv are required unless --embeddings DIR is given")
    if args.embeddings is not None and args.dump_embeddings is not None:
        parser.error("--embeddings and --dump_embeddings exclude each other")
    if args.trials < 1 or args.k < 1:
        parser.error("--trials and -k must be positive")
    if not 0.0 < args.alpha < 1.0:
        parser.error("--alpha must be in (0, 1)")
    if args.iters is not None and args.iters < 1:
        parser.error("--iters must be positive")
    if args.sigma is not None and not args.sigma > 0.0:
        parser.error("--sigma must be positive")
    return args


if __name__ == "__main__":
    main(get_args())
