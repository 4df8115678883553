"""UNFUSED encoder wrapper (`src/upstream/unfused/upstream_encoder.py:4-26` of the reference): base encoder (all layers) ->
(max + mean over time of the fc output, (x_1, x_2, x_3) the three layer means).  The shipped file unpacks the encoder's
`(x_1, x_2, x_3, x)` as `x, x_1, x_2, x_3` and dies in the classifier; this is the original's meaning
(`extras/unfused/models_delores.py:76-110`).  Module-level (autograd) path; the expert's fused step uses
the same kernels through `src.engine`."""
from torch import nn

from src.functional import MaxMeanFn


class UNFUSED(nn.Module):
    def __init__(self, config, base_encoder):
        super().__init__()
        be = config["pretrain"]["base_encoder"]
        self.encoder = base_encoder(config["pretrain"]["input"]["n_mels"], be["output_dim"], be["return_all_layers"])

    def forward(self, x):
        if repr(self.encoder) != "AudioNTT2020Task6":
            raise NotImplementedError("Unfused currently supports just AudioNTT2020Task6 encoder")
        if not self.encoder.return_all_layers:
            raise NotImplementedError("Unfused needs return_all_layers = True to be set in the config!")
        x_1, x_2, x_3, x = self.encoder(x)
        return MaxMeanFn.apply(x), (x_1, x_2, x_3)
