"""The offline labeler as one command - `main` of `extras/decar-v2/store_clusters.py:64-160` on this code base: load a checkpoint,
embed every file of a `files` CSV in eval mode without augmentation (`compute_features`, `extras/decar-v2/utils.py:75-112`),
PCA-whiten, k-means, and write the `files,label` CSV `train_upstream.py --upstream unfused` trains on.

    python -m src.upstream.decar_v2.store_clusters --checkpoint final.ckpt --upstream delores_m --input files.csv --k 585 \
        --out labelled.csv

`--window random` is the default: the reference draws `extract_window` for every clip.  Single GPU.
"""
import argparse

import pandas as pd
import torch
import yaml

from src.upstream.decar_v2.clustering import Kmeans, write_pseudolabel_csv


def main(args):
    from src.evaluation.embed import extract_embeddings, load_embedder
    if not torch.cuda.is_available():
        raise RuntimeError("store_clusters (MI355X path) needs a GPU; the HIP kernels have no CPU fallback")
    config = None
    if args.config:
        with open(args.config, "r") as f:
            config = yaml.load(f, Loader=yaml.SafeLoader)
    files = list(pd.read_csv(args.input)["files"])
    embedder = load_embedder(args.checkpoint, args.upstream, config=config, layer=args.layer)
    duration = float(embedder.model.config["pretrain"]["input"]["length_wave"])
    feats = extract_embeddings(embedder, files, batch_size=args.batch_size, window=args.window, duration=duration)
    km = Kmeans(args.k)
    loss = km.cluster(feats, verbose=args.verbose, pca=min(args.pca, feats.shape[1], max(1, len(files) - 1)))   # rank of the covariance
    labels = write_pseudolabel_csv(files, km, args.out, header="files,label")
    print(f"{len(files)} files, {args.k} clusters, k-means loss {loss:.6g} -> {args.out}")
    return labels


def get_args(argv=None):
    parser = argparse.ArgumentParser(allow_abbrev=False, description="checkpoint -> embeddings -> k-means pseudo-labels")
    parser.add_argument("--checkpoint", type=str, required=True)
    parser.add_argument("--upstream", type=str, default="delores_m")
    parser.add_argument("--input", type=str, required=True, help="csv with a `files` column")
    parser.add_argument("--k", type=int, required=True, help="number of clusters (the reference uses 585)")
    parser.add_argument("--out", type=str, required=True, help="`files,label` csv to write")
    parser.add_argument("--pca", type=int, default=128)
    parser.add_argument("--window", choices=("center", "random"), default="random")
    parser.add_argument("--layer", choices=("backbone", "head"), default="backbone")
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("-c", "--config", metavar="CONFIG_PATH", default=None)
    parser.add_argument("--verbose", action="store_true")
    return parser.parse_args(argv)


if __name__ == "__main__":
    main(get_args())
