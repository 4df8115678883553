#!/usr/bin/env python3
"""Weighted k-NN evaluation of an upstream checkpoint on the MI355X path: frozen embeddings of the train CSV are the bank, every
test clip is classified by its k nearest bank rows (cosine similarity, votes weighted by exp(sim / T)).  One pass over the
data, nothing is trained.

    python audio-ssl_amd/evaluate_knn.py --checkpoint final.ckpt --upstream delores_m --train_csv train.csv --test_csv test.csv

The CSVs are `train_downstream.py`'s (`wav,label`); label ids are sorted as `DownstreamDataset` sorts them.  Prints one JSON
line: {"top1", "k", "T", "N_train", "N_test", "d"}.  `--window whole` embeds every clip at its own length (up to `--max_duration`
seconds) instead of one `length_wave` window per file.  Single GPU.
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


def main(args):
    from src.evaluation import KnnClassifier, extract_embeddings, load_embedder
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_knn.py (MI355X path) needs a GPU; the HIP kernels have no CPU fallback")
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
    bank = extract_embeddings(embedder, list(train["wav"]), **kw)
    queries = extract_embeddings(embedder, list(test["wav"]), **kw)
    y_train = torch.tensor([label2id[v] for v in train["label"]], dtype=torch.int64)
    y_test = torch.tensor([label2id[v] for v in test["label"]], dtype=torch.int64)
    k = min(args.k, bank.shape[0])
    clf = KnnClassifier(k=k, temperature=args.temperature).fit(bank, y_train.cuda())
    top1 = clf.score(queries, y_test.cuda())
    if args.dump_embeddings:
        os.makedirs(args.dump_embeddings, exist_ok=True)
        for name, arr in (("train_embeddings", bank), ("train_labels", y_train), ("test_embeddings", queries), ("test_labels", y_test)):
            np.save(os.path.join(args.dump_embeddings, name + ".npy"), arr.cpu().numpy())
    result = dict(top1=top1, k=k, T=args.temperature, N_train=int(bank.shape[0]), N_test=int(queries.shape[0]), d=int(bank.shape[1]))
    print(json.dumps(result))
    return result


def get_args(argv=None):
    parser = argparse.ArgumentParser(allow_abbrev=False, description="weighted k-NN evaluation of an upstream checkpoint")
    parser.add_argument("--checkpoint", type=str, required=True, help="path to the pre-trained checkpoint")
    parser.add_argument("--upstream", type=str, default="delores_m")
    parser.add_argument("--train_csv", type=str, required=True, help="`wav,label` csv: the bank")
    parser.add_argument("--test_csv", type=str, required=True, help="`wav,label` csv: the queries")
    parser.add_argument("-c", "--config", metavar="CONFIG_PATH", default=None, help="yaml overriding the checkpoint's config")
    parser.add_argument("-k", type=int, default=20)
    parser.add_argument("--temperature", type=float, default=0.07)
    parser.add_argument("--layer", choices=("backbone", "head"), default="backbone")
    parser.add_argument("--window", choices=("center", "random", "whole"), default="center",
                        help="whole: every clip at its own length, in ragged batches (conv encoder)")
    parser.add_argument("--max_duration", type=float, default=30.0, help="--window whole: longer clips are centre-cropped to this many seconds")
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("--dump_embeddings", metavar="DIR", default=None, help="write embeddings and labels as .npy")
    return parser.parse_args(argv)


if __name__ == "__main__":
    main(get_args())
