from src.dataset.upstream_dataset import BaseDataset, BaselineDataModule, UpstreamFrontEnd  # noqa: F401
from src.dataset.downstream_dataset import DownstreamDataset, DownstreamDatasetHF, DownstreamFrontEnd  # noqa: F401
from src.dataset.mast_dataset import MastFrontEnd, kaldi_mel_banks, make_features, norm_stats, plan_masks  # noqa: F401
