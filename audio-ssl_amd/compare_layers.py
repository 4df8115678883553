#!/usr/bin/env python3
"""Centred kernel alignment between the layers of one checkpoint, or between the layers of two, on the MI355X path: "how similar
is layer 2 of checkpoint A to layer 3 of checkpoint B".  Every clip of the CSV goes through each model once; the n x n Gram
matrices behind CKA are never stored (src/evaluation/cka.py).

    python audio-ssl_amd/compare_layers.py --checkpoint a.ckpt --upstream delores_m --input files.csv
    python audio-ssl_amd/compare_layers.py --checkpoint a.ckpt --upstream delores_m --checkpoint_b b.ckpt --upstream_b unfused \
        --input files.csv --layers x1,x2,x3,backbone,head --kernel rbf

`files.csv` has a `files` column (the labeler's input).  Prints one JSON line {"layers_a", "layers_b", "kernel", "n", "cka"}:
cka[i][j] = CKA(layer i of A, layer j of B); with one checkpoint B = A, the matrix is symmetric with a unit diagonal.  Single GPU.
"""
import argparse
import json
import os
import sys

import pandas as pd
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def main(args):
    from src.evaluation import cka_matrix, extract_embeddings, load_embedder
    if not torch.cuda.is_available():
        raise RuntimeError("compare_layers.py (MI355X path) needs a GPU; the HIP kernels have no CPU fallback")
    layers = tuple(l for l in args.layers.split(",") if l)
    files = list(pd.read_csv(args.input)["files"])
    if args.max_files:
        files = files[:args.max_files]
    if len(files) < 2:
        raise ValueError("CKA needs at least two clips")

    def features(checkpoint, upstream):
        embedder = load_embedder(checkpoint, upstream, layer=layers)
        duration = args.duration or float(embedder.model.config["pretrain"]["input"]["length_wave"])
        return extract_embeddings(embedder, files, batch_size=args.batch_size, window=args.window, duration=duration,
                                  max_duration=args.max_duration)

    feats_a = features(args.checkpoint, args.upstream)
    feats_b = features(args.checkpoint_b, args.upstream_b or args.upstream) if args.checkpoint_b else None
    m = cka_matrix(feats_a, feats_b, kernel=args.kernel, sigma=args.sigma)
    result = dict(layers_a=list(layers), layers_b=list(layers), kernel=args.kernel, n=len(files), cka=m.tolist())
    print(json.dumps(result))
    return result


def get_args(argv=None):
    parser = argparse.ArgumentParser(allow_abbrev=False, description="CKA between the layers of one or two upstream checkpoints")
    parser.add_argument("--checkpoint", type=str, required=True, help="checkpoint A")
    parser.add_argument("--upstream", type=str, default="delores_m", help="upstream of checkpoint A")
    parser.add_argument("--checkpoint_b", type=str, default=None, help="checkpoint B (default: A against itself)")
    parser.add_argument("--upstream_b", type=str, default=None, help="upstream of checkpoint B (default: --upstream)")
    parser.add_argument("--input", type=str, required=True, help="csv with a `files` column")
    parser.add_argument("--layers", type=str, default="x1,x2,x3,backbone,head")
    parser.add_argument("--kernel", choices=("linear", "rbf"), default="linear")
    parser.add_argument("--sigma", type=float, default=None, help="RBF width for both matrices (default: median rule per matrix)")
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("--duration", type=float, default=None, help="seconds per clip (default: the checkpoint's length_wave)")
    parser.add_argument("--max_files", type=int, default=None)
    parser.add_argument("--window", choices=("center", "whole"), default="center",
                        help="whole: every clip at its own length, in ragged batches (conv encoder)")
    parser.add_argument("--max_duration", type=float, default=30.0, help="--window whole: longer clips are centre-cropped to this many seconds")
    return parser.parse_args(argv)


if __name__ == "__main__":
    main(get_args())
