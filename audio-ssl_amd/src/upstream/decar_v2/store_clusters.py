"""The offline labeler as one command - `main` of `extras/decar-v2/store_clusters.py:64-160` on this code base: load a checkpoint,
embed every file of a `files` CSV in eval mode without augmentation (`compute_features`, `extras/decar-v2/utils.py:75-112`),
PCA-whiten, cluster, and write the `files,label` CSV `train_upstream.py --upstream unfused` trains on.

    python -m src.upstream.decar_v2.store_clusters --checkpoint final.ckpt --upstream delores_m --input files.csv --k 585 \
        --out labelled.csv
    python -m src.upstream.decar_v2.store_clusters --checkpoint final.ckpt --upstream delores_m --input files.csv \
        --clustering pic --out labelled.csv

`--clustering kmeans` (the default) needs `--k`.  `--clustering pic` is the reference's other algorithm (`PIC`, imported next to
`Kmeans` at `store_clusters.py:18`): power-iteration clustering on an exact nearest-neighbour graph, which finds the number of
clusters itself; the summary line prints that number, which is what `pretrain.task_label` has to be set to.
`--compare other.csv` prints the normalised mutual information between the labels just written and those of another
`files,label` file over the same files (a k-means labeling against a PIC one, or pseudo-labels against real ones).
`--window random` is the default: the reference draws `extract_window` for every clip.  Single GPU.
"""
import argparse
import sys

import pandas as pd
import torch
import yaml

from src.upstream.decar_v2.clustering import PIC, Kmeans, write_pseudolabel_csv


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
    pca = min(args.pca, feats.shape[1], max(1, len(files) - 1))                                  # rank of the covariance
    if args.clustering == "pic":
        if args.k is not None:
            print("warning: --k is ignored with --clustering pic (the number of clusters is found)", file=sys.stderr)
        model = PIC(sigma=args.sigma, nnn=args.nnn, alpha=args.alpha, distribute_singletons=not args.no_distribute_singletons)
        model.cluster(feats, verbose=args.verbose, pca=pca)
        labels = write_pseudolabel_csv(files, model, args.out, header="files,label")
        print(f"{len(files)} files, {len(model.images_lists)} clusters, pic sigma {args.sigma:g} nnn {args.nnn} -> {args.out}")
    else:
        model = Kmeans(args.k)
        loss = model.cluster(feats, verbose=args.verbose, pca=pca)
        labels = write_pseudolabel_csv(files, model, args.out, header="files,label")
        print(f"{len(files)} files, {args.k} clusters, k-means loss {loss:.6g} -> {args.out}")
    if args.compare:
        from src.evaluation.graph import partition_nmi
        other = pd.read_csv(args.compare)
        if list(other["files"]) != files:
            raise ValueError(f"{args.compare} does not list the files of {args.input} in the same order")
        codes = pd.factorize(other["label"])[0]
        print(f"NMI against {args.compare}: {partition_nmi(labels, codes):.6f}")
    return labels


def get_args(argv=None):
    parser = argparse.ArgumentParser(allow_abbrev=False, description="checkpoint -> embeddings -> k-means or PIC pseudo-labels")
    parser.add_argument("--checkpoint", type=str, required=True)
    parser.add_argument("--upstream", type=str, default="delores_m")
    parser.add_argument("--input", type=str, required=True, help="csv with a `files` column")
    parser.add_argument("--clustering", choices=("kmeans", "pic"), default="kmeans")
    parser.add_argument("--k", type=int, default=None, help="number of clusters for k-means (the reference uses 585); ignored by pic")
    parser.add_argument("--out", type=str, required=True, help="`files,label` csv to write")
    parser.add_argument("--pca", type=int, default=128)
    parser.add_argument("--sigma", type=float, default=0.2, help="pic: bandwidth of the Gaussian kernel")
    parser.add_argument("--nnn", type=int, default=5, help="pic: nearest neighbours per node")
    parser.add_argument("--alpha", type=float, default=0.001, help="pic: damping of the power iteration")
    parser.add_argument("--no_distribute_singletons", action="store_true", help="pic: keep one-member clusters")
    parser.add_argument("--compare", type=str, default=None, help="another `files,label` csv: print the NMI against it")
    parser.add_argument("--window", choices=("center", "random"), default="random")
    parser.add_argument("--layer", choices=("backbone", "head"), default="backbone")
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("-c", "--config", metavar="CONFIG_PATH", default=None)
    parser.add_argument("--verbose", action="store_true")
    args = parser.parse_args(argv)
    if args.clustering == "kmeans" and args.k is None:
        parser.error("the following arguments are required: --k")       # argparse's own wording for a required option
    return args


if __name__ == "__main__":
    main(get_args())
