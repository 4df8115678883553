"""What a user does with a checkpoint: embeddings (`embed`), k-NN evaluation (`knn`), layer similarity (`cka`), multi-label tagging loss
and metrics (`tagging`), exact neighbour graphs, partition scores and the silhouette of a labeling (`graph`), a 2-D t-SNE map of the features (`tsne`), linear evaluation with a grid of heads trained
in one pass (`probe`), low-shot evaluation and seeded pseudo-labels by label spreading on the neighbour graph (`spread`),
near-duplicate and leakage search by an exact radius graph and its connected components (`dedup`), HDBSCAN on the exact
mutual-reachability spanning tree - clusters of any density and a noise label (`hdbscan`; the function of that name is
`src.evaluation.hdbscan.hdbscan`, the package attribute stays the module)."""
from src.evaluation.cka import cka_matrix, hsic_terms, kernel_cka, linear_cka, median_sigma2  # noqa: F401
from src.evaluation.dedup import (Duplicates, RangeCsr, cosine_to_radius2, graph_components, near_duplicates, range_graph,  # noqa: F401
                                  range_search, select_keep)
from src.evaluation.embed import (Embedder, center_start, extract_embeddings, load_embedder, plan_ragged_batches,  # noqa: F401
                                  take_window)
from src.evaluation.graph import knn_graph, partition_nmi, silhouette_samples, silhouette_score  # noqa: F401
from src.evaluation.hdbscan import (HdbscanResult, MstEdges, condense_tree, core_distances2, cut_mst,  # noqa: F401
                                    mutual_reachability_mst, select_eom, single_linkage)
from src.evaluation.knn import KnnClassifier, knn_predict, knn_topk, knn_topk_bf16, normalize_bf16  # noqa: F401
from src.evaluation.probe import (LinearProbeGrid, cosine_scale, epoch_permutations, feature_stats, fold_standardisation,  # noqa: F401
                                  head_index, select_head, stratified_holdout)
from src.evaluation.spread import (SpreadResult, label_spread, lowshot_evaluate, lowshot_seeds, spread_assign,  # noqa: F401
                                   spread_normalize)
from src.evaluation.tagging import (bce_with_logits, build_class_index, mix_labels, multi_hot, parse_labels,  # noqa: F401
                                    tagging_stats)
from src.evaluation.tsne import tsne, tsne_affinities, tsne_gradient  # noqa: F401
