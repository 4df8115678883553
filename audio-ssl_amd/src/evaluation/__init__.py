"""What a user does with a checkpoint: embeddings (`embed`), k-NN evaluation (`knn`)."""
from src.evaluation.embed import Embedder, center_start, extract_embeddings, load_embedder, take_window  # noqa: F401
from src.evaluation.knn import KnnClassifier, knn_predict, knn_topk, knn_topk_bf16, normalize_bf16  # noqa: F401
