#!/usr/bin/env python3
"""Near-duplicate search in a file list, and leakage check between two, on the MI355X path: the files are embedded with a frozen
checkpoint, every pair of embeddings with cosine similarity >= `--threshold` is found EXACTLY (a radius graph, not a top-k list:
a group of 3,000 re-uploads is found whole), and the graph's connected components are the duplicate groups.

    python audio-ssl_amd/find_duplicates.py --checkpoint final.ckpt --upstream delores_m --input files.csv --out kept.csv --groups groups.csv
    python audio-ssl_amd/find_duplicates.py --checkpoint final.ckpt --upstream delores_m --input train.csv --against test.csv --out clean.csv

The path column of a CSV is `files` if present, else `wav`; every other column of `--input` is carried into `--out`, so a
`wav,label` file stays a `train_downstream.py` input and a `files` file a `train_upstream.py --input`.

Without `--against`: `--out` holds the kept rows of `--input` in input order (one per group: `--keep first` the first of the
group, `central` the one with the most matches); `--groups` one line per file in a group of two or more
(`files,group,size,kept,nearest,similarity`).  Groups are single-linkage: A~B and B~C put A and C together.
With `--against`: the leakage check.  `--out` holds the `--input` rows with no match among the `--against` files; `--groups` lists
each leaking file (`files,matches,nearest,similarity`: its nearest `--against` file).

Prints one JSON line: {"N", "N_against", "threshold", "edges", "groups", "removed", "largest_group", "max_degree", "d"} (with
`--against`: groups = leaking files, largest_group = the most `--against` files one input file matches).
`--embeddings X.npy` ([N, d] float32, rows in `--input` order; `--against_embeddings` likewise) skips the checkpoint.  The window
is deterministic (`center` or `whole`).  This finds duplicates in embedding space at the chosen window, not audio fingerprints.
Single GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import pandas as pd
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

GROUP_COLUMNS = ["files", "group", "size", "kept", "nearest", "similarity"]
LEAK_COLUMNS = ["files", "matches", "nearest", "similarity"]


def path_column(frame, name):
    """The column of a CSV that holds the paths: `files` if present, else `wav`."""
    for c in ("files", "wav"):
        if c in frame.columns:
            return c
    raise ValueError(f"{name} has neither a `files` nor a `wav` column (columns: {list(frame.columns)})")


def check_args(args):
    """Argument combinations that cannot work, refused before anything is read or launched."""
    if not 0.0 < args.threshold <= 1.0:
        raise ValueError(f"--threshold is a cosine similarity in (0, 1], got {args.threshold}")
    if args.embeddings is None and args.checkpoint is None:
        raise ValueError("give --checkpoint (embed the files) or --embeddings (use stored rows)")
    if args.against_embeddings is not None and args.against is None:
        raise ValueError("--against_embeddings needs --against")
    if args.against_embeddings is not None and args.embeddings is None:
        raise ValueError("--against_embeddings needs --embeddings")
    if args.embeddings is not None and args.against is not None and args.against_embeddings is None:
        raise ValueError("--embeddings with --against needs --against_embeddings")
    if args.embeddings is not None and args.dump_embeddings is not None:
        raise ValueError("--embeddings and --dump_embeddings exclude each other")
    if args.max_edges is not None and args.max_edges < 0:
        raise ValueError(f"--max_edges must be >= 0, got {args.max_edges}")


def load_rows(path, n, what):
    arr = np.load(path, allow_pickle=False)
    if arr.ndim != 2 or arr.shape[0] != n:
        raise ValueError(f"{path} holds an array of shape {arr.shape}; {what} has {n} rows, so [{n}, d] is needed")
    return np.ascontiguousarray(arr, dtype=np.float32)


def write_kept(frame, keep, out):
    """The rows of `frame` that stay, in input order, every column carried through."""
    frame[np.asarray(keep, dtype=bool)].to_csv(out, index=False)


def write_groups(paths, dup, out):
    """One line per file in a group of two or more, in input order."""
    rows = np.flatnonzero(np.asarray(dup.size) >= 2)
    pd.DataFrame({"files": [paths[i] for i in rows], "group": dup.group[rows], "size": dup.size[rows],
                  "kept": dup.keep[rows].astype(int), "nearest": [paths[dup.nearest[i]] for i in rows],
                  "similarity": dup.nearest_sim[rows]}, columns=GROUP_COLUMNS).to_csv(out, index=False)


def write_leaks(paths, against_paths, degree, nearest, similarity, out):
    """One line per `--input` file with a match among the `--against` files, in input order."""
    rows = np.flatnonzero(np.asarray(degree) > 0)
    pd.DataFrame({"files": [paths[i] for i in rows], "matches": np.asarray(degree)[rows],
                  "nearest": [against_paths[nearest[i]] for i in rows], "similarity": np.asarray(similarity)[rows]},
                 columns=LEAK_COLUMNS).to_csv(out, index=False)


def main(args):
    check_args(args)
    frame = pd.read_csv(args.input)
    col = path_column(frame, args.input)
    paths = list(frame[col])
    other, other_paths = None, None
    if args.against:
        other = pd.read_csv(args.against)
        other_paths = list(other[path_column(other, args.against)])
    if args.embeddings:
        x = load_rows(args.embeddings, len(paths), args.input)
        y = load_rows(args.against_embeddings, len(other_paths), args.against) if args.against else None
        if y is not None and y.shape[1] != x.shape[1]:
            raise ValueError(f"{args.embeddings} has width {x.shape[1]}, {args.against_embeddings} has {y.shape[1]}")
    if not torch.cuda.is_available():
        raise RuntimeError("find_duplicates.py (MI355X path) needs a GPU; the HIP kernels have no CPU fallback")
    from src.evaluation import dedup as D
    if args.embeddings:
        x = torch.from_numpy(x).cuda()
        y = torch.from_numpy(y).cuda() if y is not None else None
    else:
        from src.evaluation import extract_embeddings, load_embedder
        config = None
        if args.config:
            with open(args.config, "r") as f:
                config = yaml.load(f, Loader=yaml.SafeLoader)
        embedder = load_embedder(args.checkpoint, args.upstream, config=config, layer=args.layer)
        duration = float(embedder.model.config["pretrain"]["input"]["length_wave"])
        kw = dict(batch_size=args.batch_size, window=args.window, duration=duration, max_duration=args.max_duration)
        x = extract_embeddings(embedder, paths, **kw).float()
        y = extract_embeddings(embedder, other_paths, **kw).float() if args.against else None
        if args.dump_embeddings:
            os.makedirs(args.dump_embeddings, exist_ok=True)
            np.save(os.path.join(args.dump_embeddings, "input_embeddings.npy"), x.cpu().numpy())
            if y is not None:
                np.save(os.path.join(args.dump_embeddings, "against_embeddings.npy"), y.cpu().numpy())
    unit = lambda t: t / t.norm(dim=1, keepdim=True).clamp_min(1e-30)       # noqa: E731
    n = len(paths)
    if args.against:
        csr = D.range_search(unit(x), unit(y), D.cosine_to_radius2(args.threshold), max_edges=args.max_edges)
        degree = (csr.rowptr[1:] - csr.rowptr[:-1]).long()
        nearest, best = D.row_nearest(csr, n)
        degree, nearest, sim = degree.cpu().numpy(), nearest.cpu().numpy(), (1.0 - 0.5 * best.double()).cpu().numpy()
        write_kept(frame, degree == 0, args.out)
        if args.groups:
            write_leaks(paths, other_paths, degree, nearest, sim, args.groups)
        leaking = int((degree > 0).sum())
        result = dict(N=n, N_against=len(other_paths), threshold=args.threshold, edges=int(csr.col.numel()), groups=leaking,
                      removed=leaking, largest_group=int(degree.max()), max_degree=int(degree.max()), d=int(x.shape[1]))
    else:
        dup = D.near_duplicates(x, threshold=args.threshold, metric="cosine", keep=args.keep, max_edges=args.max_edges)
        write_kept(frame, dup.keep, args.out)
        if args.groups:
            write_groups(paths, dup, args.groups)
        result = dict(N=n, N_against=0, threshold=args.threshold, edges=int(dup.csr.col.numel()),
                      groups=int((np.bincount(dup.group, minlength=dup.n_groups) >= 2).sum()), removed=int((~dup.keep).sum()),
                      largest_group=int(dup.size.max()), max_degree=int(dup.degree.max()), d=int(x.shape[1]))
    print(json.dumps(result))
    return result


def get_args(argv=None):
    parser = argparse.ArgumentParser(allow_abbrev=False, description="near-duplicate / leakage search on frozen embeddings")
    parser.add_argument("--checkpoint", type=str, default=None, help="path to the pre-trained checkpoint")
    parser.add_argument("--upstream", type=str, default="delores_m")
    parser.add_argument("--input", type=str, required=True, help="csv with a `files` or `wav` column: the list to clean")
    parser.add_argument("--against", type=str, default=None, help="csv of the other split: report --input files that match one of these")
    parser.add_argument("-c", "--config", metavar="CONFIG_PATH", default=None, help="yaml overriding the checkpoint's config")
    parser.add_argument("--threshold", type=float, default=0.98, help="cosine similarity from which two clips match")
    parser.add_argument("--keep", choices=("first", "central"), default="first")
    parser.add_argument("--window", choices=("center", "whole"), default="center",
                        help="whole: every clip at its own length, in ragged batches (conv encoder)")
    parser.add_argument("--max_duration", type=float, default=30.0, help="--window whole: longer clips are centre-cropped to this many seconds")
    parser.add_argument("--layer", choices=("backbone", "head"), default="backbone")
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("--embeddings", metavar="X.npy", default=None, help="[N, d] float32, rows in --input order: no checkpoint needed")
    parser.add_argument("--against_embeddings", metavar="Y.npy", default=None, help="the same for --against")
    parser.add_argument("--dump_embeddings", metavar="DIR", default=None, help="write the embeddings as .npy")
    parser.add_argument("--max_edges", type=int, default=None, help="refuse a graph with more matches (default 64 per file)")
    parser.add_argument("--out", type=str, required=True, help="csv of the rows of --input that stay")
    parser.add_argument("--groups", type=str, default=None, help="csv listing the duplicate groups / the leaking files")
    return parser.parse_args(argv)


if __name__ == "__main__":
    main(get_args())
