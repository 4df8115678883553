"""The offline labeler as one command - `main` of `extras/decar-v2/store_clusters.py:64-160` on this code base: load a checkpoint,
embed every file of a `files` CSV in eval mode without augmentation (`compute_features`, `extras/decar-v2/utils.py:75-112`),
PCA-whiten, cluster, and write the `files,label` CSV `train_upstream.py --upstream unfused` trains on.

    python -m src.upstream.decar_v2.store_clusters --checkpoint final.ckpt --upstream delores_m --input files.csv --k 585 \
        --out labelled.csv
    python -m src.upstream.decar_v2.store_clusters --checkpoint final.ckpt --upstream delores_m --input files.csv \
        --clustering pic --score --out labelled.csv
    python -m src.upstream.decar_v2.store_clusters --checkpoint final.ckpt --upstream delores_m --input files.csv \
        --k_sweep 64,128,256 --out labelled.csv
    python -m src.upstream.decar_v2.store_clusters --checkpoint final.ckpt --upstream delores_m --input files.csv --k 585 \
        --out labelled.csv --map map.csv
    python -m src.upstream.decar_v2.store_clusters --checkpoint final.ckpt --upstream delores_m --input files.csv \
        --clustering spread --seed_labels few.csv --drop_unreached --out labelled.csv
    python -m src.upstream.decar_v2.store_clusters --checkpoint final.ckpt --upstream delores_m --input files.csv \
        --clustering hdbscan --min_cluster_size 25 --min_samples 5 --drop_unreached --out labelled.csv

`--clustering kmeans` (the default) needs `--k`.  `--clustering pic` is the reference's other algorithm (`PIC`, imported next to
`Kmeans` at `store_clusters.py:18`): power-iteration clustering on an exact nearest-neighbour graph, which finds the number of
clusters itself; the summary line prints that number, which is what `pretrain.task_label` has to be set to.
`--clustering spread --seed_labels few.csv` is for the user who HAS labels for a few files: `few.csv` is a `files,label` CSV whose
files are a subset of `--input`; its label values, sorted as strings, become the ids 0 .. C - 1 (the mapping is printed) and label
spreading (`src.evaluation.spread.label_spread`, Zhou et al. 2004) carries them over the exact nearest-neighbour graph of the
whitened features (`--nnn`, `--sigma`; `--spread_alpha`, `--spread_iters`) to every other file, so the ids written ARE the
user's classes.  Seed files keep the label they came with.  A file no seed reaches is written with label -1 and counted in the
summary line; `--drop_unreached` leaves those files out of `--out` (UnFuSeD needs 0 .. C - 1); `--confidence` adds a third column,
1 - H(p) / log C of the file's class distribution.  The reference has no counterpart.
`--clustering hdbscan` is for file lists full of clips that belong NOWHERE (MUSAN, web crawls): every other algorithm here forces
each of them into a cluster, and each becomes a wrong pseudo-label.  HDBSCAN (`src.evaluation.hdbscan.hdbscan`: the exact
mutual-reachability spanning tree on the GPU, `--min_cluster_size`, `--min_samples`) needs no `--k`, finds the number of clusters
(printed; it is `pretrain.task_label`), copes with clusters of different density and labels the rest -1.  Those rows are written
unless `--drop_unreached` is given (UnFuSeD needs 0 .. C - 1); `--confidence` adds the membership strength as a third column;
`--score` scores the files that are in a cluster.  The reference has no counterpart.
`--compare other.csv` prints the normalised mutual information between the labels just written and those of another
`files,label` file over the same files (a k-means labeling against a PIC one, or pseudo-labels against real ones).
`--score` prints the silhouette coefficient (sklearn's `silhouette_score`, Euclidean) of the labels just written on the whitened
features they were computed on: the label-free answer to "is this labeling any good" (`src.evaluation.graph.silhouette_score`,
all pairs on the GPU, no distance matrix stored).  `--k_sweep 64,128,256` takes the place of `--k`: the files are embedded and
whitened once, k-means runs for every k in the order given, one line per k reports its silhouette, and the labeling with the
highest silhouette (a tie: the smaller k) is written; the reference has neither.
`--map map.csv` draws the picture that goes with the numbers: a 2-D t-SNE layout (`src.evaluation.tsne.tsne`, exact repulsion on
the GPU, `--perplexity` up to 21, `--map_iters` iterations) of the same whitened features, written as `files,label,x,y` for any
plotting tool to colour by label; one more line reports the final KL divergence.
`--window random` is the default: the reference draws `extract_window` for every clip; `--window whole` embeds every clip at its
own length (up to `--max_duration` seconds).  Single GPU.
"""
import argparse
import sys

import numpy as np
import pandas as pd
import torch
import yaml

from src.upstream.decar_v2.clustering import PIC, Kmeans, preprocess_features, run_kmeans, write_pseudolabel_csv


def _silhouette(features, labels):
    """-> (score or None when the labeling has fewer than 2 or more than n - 1 clusters, clusters, one-member clusters)"""
    from src.evaluation.graph import silhouette_score
    sizes = np.unique(np.asarray(labels), return_counts=True)[1]
    ok = 2 <= len(sizes) <= len(labels) - 1
    return (silhouette_score(features, labels) if ok else None), len(sizes), int((sizes == 1).sum())


def _fmt(score):
    return "n/a" if score is None else f"{score:.6f}"


def sweep_kmeans(feats, ks, pca, verbose=False):
    """k-means for every k of `ks` on the same whitened features -> the `Kmeans` of the k with the highest silhouette (a tie: the
    smaller k), its loss and its silhouette; one table line per k.  The seeds are the draws successive `Kmeans(k).cluster` calls
    would make."""
    xb = preprocess_features(feats, pca=pca)
    n = xb.shape[0]
    if max(ks) > n:
        raise ValueError(f"--k_sweep: k = {max(ks)} exceeds the {n} files")
    best = None
    for k in ks:
        I, loss = run_kmeans(xb, k, verbose)
        score, used, _ = _silhouette(xb, I)
        print(f"k {k}: {used} non-empty clusters, k-means loss {loss:.6g}, silhouette {_fmt(score)}")
        if score is not None and (best is None or score > best[0] or (score == best[0] and k < best[1])):
            best = (score, k, I, loss)
    if best is None:
        raise ValueError("--k_sweep: no k gave a labeling with 2 .. n - 1 non-empty clusters, nothing to choose from")
    score, k, I, loss = best
    model = Kmeans(k)
    model.features = xb
    model.images_lists = [[] for _ in range(k)]
    for i, c in enumerate(I):
        model.images_lists[c].append(i)
    return model, loss, score


def read_seed_labels(path, files):
    """`files,label` CSV whose files are a subset of `files` -> (row of every seed in `files`, its class id, class names): label
    values sorted as strings become 0 .. C - 1.  Anything else is a ValueError naming the first offender."""
    few = pd.read_csv(path)
    for column in ("files", "label"):
        if column not in few.columns:
            raise ValueError(f"{path} has no `{column}` column")
    if len(few) == 0:
        raise ValueError(f"{path} lists no file")
    where = {}
    for i, f in enumerate(files):
        where.setdefault(f, i)
    names = sorted(set(few["label"]), key=str)
    label2id = {k: i for i, k in enumerate(names)}
    rows, ids, seen = [], [], set()
    for f, v in zip(few["files"], few["label"]):
        if f not in where:
            raise ValueError(f"{path}: {f} is not a file of --input")
        if f in seen:
            raise ValueError(f"{path}: {f} is listed more than once")
        seen.add(f)
        rows.append(where[f])
        ids.append(label2id[v])
    return np.asarray(rows, dtype=np.int64), np.asarray(ids, dtype=np.int64), [str(k) for k in names]


def spread_labels(feats, rows, ids, classes, pca, nnn, sigma, alpha, iters=None):
    """-> (whitened features, label per file as int64 numpy with -1 = unreached, confidence per file): one trial of label spreading
    from the seeds (rows, ids) on the graph PIC would build; seeds keep their label."""
    from src.evaluation.graph import knn_graph, pic_build
    from src.evaluation.spread import label_spread
    xb = preprocess_features(feats, pca=pca)
    idx, d2 = knn_graph(xb, min(nnn, xb.shape[0] - 1))
    W = pic_build(idx, d2, sigma)
    res = label_spread(W, torch.from_numpy(rows), torch.from_numpy(ids), classes, classes, alpha=alpha, iters=iters)
    labels = res.labels[:, 0].cpu().numpy().astype(np.int64)
    labels[rows] = ids
    return xb, labels, res.confidence[:, 0].cpu().numpy()


def write_labels_with_unreached(files, labels, conf, args):
    """`files,label[,confidence]` to args.out for the algorithms that may leave a file without a label (-1): spread, hdbscan."""
    with open(args.out, "w") as f:
        f.write("files,label,confidence\n" if args.confidence else "files,label\n")
        for p, l, c in zip(files, labels, conf):
            if l >= 0 or not args.drop_unreached:
                f.write(f"{p},{int(l)},{float(c):.6f}\n" if args.confidence else f"{p},{int(l)}\n")


def main(args):
    from src.evaluation.embed import extract_embeddings, load_embedder
    if not torch.cuda.is_available():
        raise RuntimeError("store_clusters (MI355X path) needs a GPU; the HIP kernels have no CPU fallback")
    config = None
    if args.config:
        with open(args.config, "r") as f:
            config = yaml.load(f, Loader=yaml.SafeLoader)
    files = list(pd.read_csv(args.input)["files"])
    if args.clustering == "spread":
        seed_rows, seed_ids, names = read_seed_labels(args.seed_labels, files)       # a bad seed file: refused before the embedding
    if args.map:
        from src.evaluation.tsne import neighbour_count
        neighbour_count(len(files), args.perplexity)                     # a perplexity the map cannot have: refused before the embedding
    embedder = load_embedder(args.checkpoint, args.upstream, config=config, layer=args.layer)
    duration = float(embedder.model.config["pretrain"]["input"]["length_wave"])
    feats = extract_embeddings(embedder, files, batch_size=args.batch_size, window=args.window, duration=duration,
                               max_duration=args.max_duration)
    pca = min(args.pca, feats.shape[1], max(1, len(files) - 1))                                  # rank of the covariance
    chosen = None
    if args.clustering == "pic":
        if args.k is not None:
            print("warning: --k is ignored with --clustering pic (the number of clusters is found)", file=sys.stderr)
        model = PIC(sigma=args.sigma, nnn=args.nnn, alpha=args.alpha, distribute_singletons=not args.no_distribute_singletons)
        model.cluster(feats, verbose=args.verbose, pca=pca)
        labels = write_pseudolabel_csv(files, model, args.out, header="files,label")
        print(f"{len(files)} files, {len(model.images_lists)} clusters, pic sigma {args.sigma:g} nnn {args.nnn} -> {args.out}")
        features = model.features
    elif args.clustering == "spread":
        print("classes: " + ", ".join(f"{i}={name}" for i, name in enumerate(names)))
        features, labels, conf = spread_labels(feats, seed_rows, seed_ids, len(names), pca, args.nnn, args.sigma, args.spread_alpha,
                                               args.spread_iters)
        unreached = int((labels < 0).sum())
        write_labels_with_unreached(files, labels, conf, args)
        print(f"{len(files)} files, {len(names)} classes from {len(seed_rows)} seeds, {unreached} unreached"
              f"{' (dropped)' if args.drop_unreached else ''}, spread sigma {args.sigma:g} nnn {args.nnn} alpha {args.spread_alpha:g} -> {args.out}")
    elif args.clustering == "hdbscan":
        from src.evaluation.hdbscan import hdbscan
        features = preprocess_features(feats, pca=pca)
        res = hdbscan(features, min_cluster_size=args.min_cluster_size, min_samples=args.min_samples)
        labels, conf = res.labels, res.probabilities
        noise = int((labels < 0).sum())
        write_labels_with_unreached(files, labels, conf, args)
        print(f"{len(files)} files, {res.n_clusters} clusters, {noise} noise{' (dropped)' if args.drop_unreached else ''}, hdbscan "
              f"min_cluster_size {args.min_cluster_size} min_samples {args.min_samples} -> {args.out}")
    else:
        if args.k_sweep:
            model, loss, chosen = sweep_kmeans(feats, args.k_sweep, pca, verbose=args.verbose)
        else:
            model = Kmeans(args.k)
            loss = model.cluster(feats, verbose=args.verbose, pca=pca)
        labels = write_pseudolabel_csv(files, model, args.out, header="files,label")
        print(f"{len(files)} files, {model.k} clusters, k-means loss {loss:.6g} -> {args.out}")
        features = model.features
    if args.score:
        if args.clustering == "hdbscan":                                 # noise is in no cluster: the files that are in one
            inside = np.flatnonzero(labels >= 0)
            score, count, singles = (_silhouette(features[torch.from_numpy(inside).to(features.device)], labels[inside])
                                     if len(inside) else (None, 0, 0))
        else:
            score, count, singles = _silhouette(features, labels)
        print(f"silhouette {_fmt(score)} ({count} clusters, {singles} singletons)")
    if args.map:
        from src.evaluation.tsne import tsne
        y, kl = tsne(features, perplexity=args.perplexity, n_iter=args.map_iters, return_kl=True)
        y = y.cpu().numpy()
        pd.DataFrame({"files": files, "label": [int(c) for c in labels], "x": y[:, 0], "y": y[:, 1]}).to_csv(args.map, index=False)
        print(f"map of {len(files)} files, perplexity {args.perplexity:g}, {args.map_iters} iterations, KL {kl:.6f} -> {args.map}")
    if args.compare:
        from src.evaluation.graph import partition_nmi
        other = pd.read_csv(args.compare)
        if list(other["files"]) != files:
            raise ValueError(f"{args.compare} does not list the files of {args.input} in the same order")
        codes = pd.factorize(other["label"])[0]
        print(f"NMI against {args.compare}: {partition_nmi(labels, codes):.6f}")
    if chosen is not None:
        print(f"chosen k {model.k} of {','.join(str(k) for k in args.k_sweep)} (silhouette {chosen:.6f})")
    return labels


def _k_list(text):
    try:
        ks = [int(t) for t in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"a comma-separated list of integers, got {text!r}")
    if not ks or min(ks) < 1:
        raise argparse.ArgumentTypeError(f"every k must be at least 1, got {text!r}")
    return ks


def get_args(argv=None):
    parser = argparse.ArgumentParser(allow_abbrev=False, description="checkpoint -> embeddings -> k-means, PIC, seeded (label spreading) or HDBSCAN pseudo-labels")
    parser.add_argument("--checkpoint", type=str, required=True)
    parser.add_argument("--upstream", type=str, default="delores_m")
    parser.add_argument("--input", type=str, required=True, help="csv with a `files` column")
    parser.add_argument("--clustering", choices=("kmeans", "pic", "spread", "hdbscan"), default="kmeans")
    parser.add_argument("--k", type=int, default=None, help="number of clusters for k-means (the reference uses 585); ignored by pic")
    parser.add_argument("--k_sweep", type=_k_list, default=None,
                        help="k-means: comma-separated k values in place of --k; the k with the highest silhouette is written")
    parser.add_argument("--out", type=str, required=True, help="`files,label` csv to write")
    parser.add_argument("--pca", type=int, default=128)
    parser.add_argument("--sigma", type=float, default=0.2, help="pic, spread: bandwidth of the Gaussian kernel")
    parser.add_argument("--nnn", type=int, default=5, help="pic, spread: nearest neighbours per node")
    parser.add_argument("--alpha", type=float, default=0.001, help="pic: damping of the power iteration")
    parser.add_argument("--no_distribute_singletons", action="store_true", help="pic: keep one-member clusters")
    parser.add_argument("--seed_labels", type=str, default=None, help="spread: `files,label` csv of the labelled files (a subset of --input)")
    parser.add_argument("--spread_alpha", type=float, default=0.99, help="spread: share of a node's value that comes from its neighbours")
    parser.add_argument("--spread_iters", type=int, default=None, help="spread: rounds (default: until spread_alpha^iters <= 1e-3)")
    parser.add_argument("--drop_unreached", action="store_true", help="spread: leave files no seed reaches out of --out; hdbscan: the noise files")
    parser.add_argument("--confidence", action="store_true", help="spread: a third column, 1 - H(p) / log C; hdbscan: the membership strength")
    parser.add_argument("--min_cluster_size", type=int, default=25, help="hdbscan: the smallest group that counts as a cluster")
    parser.add_argument("--min_samples", type=int, default=5, help="hdbscan: the neighbour (the file itself counted) whose distance is a file's core distance")
    parser.add_argument("--compare", type=str, default=None, help="another `files,label` csv: print the NMI against it")
    parser.add_argument("--score", action="store_true", help="print the silhouette coefficient of the labels just written")
    parser.add_argument("--map", type=str, default=None, help="`files,label,x,y` csv to write: a 2-D t-SNE map of the whitened features")
    parser.add_argument("--perplexity", type=float, default=20.0, help="--map: t-SNE perplexity, 1 .. 21")
    parser.add_argument("--map_iters", type=int, default=1000, help="--map: t-SNE iterations")
    parser.add_argument("--window", choices=("center", "random", "whole"), default="random",
                        help="whole: every clip at its own length, in ragged batches (conv encoder)")
    parser.add_argument("--max_duration", type=float, default=30.0, help="--window whole: longer clips are centre-cropped to this many seconds")
    parser.add_argument("--layer", choices=("backbone", "head"), default="backbone")
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("-c", "--config", metavar="CONFIG_PATH", default=None)
    parser.add_argument("--verbose", action="store_true")
    args = parser.parse_args(argv)
    if args.k_sweep is not None and args.k is not None:
        parser.error("--k_sweep takes the place of --k: give one of them")
    if args.k_sweep is not None and args.clustering == "pic":
        parser.error("--k_sweep is for k-means: pic finds the number of clusters itself")
    if args.clustering == "hdbscan":
        if args.k is not None or args.k_sweep is not None:
            parser.error("--k and --k_sweep are for k-means: hdbscan finds the number of clusters itself")
        if args.min_cluster_size < 2:
            parser.error("--min_cluster_size must be at least 2")
        if not 1 <= args.min_samples <= 65:
            parser.error("--min_samples must be in 1 .. 65")
    if args.clustering == "spread":
        if args.k is not None or args.k_sweep is not None:
            parser.error("--k and --k_sweep are for k-means: spread takes its classes from --seed_labels")
        if args.seed_labels is None:
            parser.error("--clustering spread needs --seed_labels")
        if not 0.0 < args.spread_alpha < 1.0:
            parser.error("--spread_alpha must be in (0, 1)")
        if args.spread_iters is not None and args.spread_iters < 1:
            parser.error("--spread_iters must be positive")
    elif args.seed_labels is not None:
        parser.error("--seed_labels goes with --clustering spread")
    elif args.clustering != "hdbscan" and (args.drop_unreached or args.confidence):
        parser.error("--seed_labels, --drop_unreached and --confidence go with --clustering spread (the last two also with hdbscan)")
    if args.clustering == "kmeans" and args.k is None and args.k_sweep is None:
        parser.error("the following arguments are required: --k")       # argparse's own wording for a required option
    return args


if __name__ == "__main__":
    main(get_args())
