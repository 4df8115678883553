#!/usr/bin/env python3
"""Generate `step_unfused.npz` by RUNNING THE REFERENCE's UnFuSeD expert on the CPU (build container only, like make_goldens.py):

    python tests/golden/make_unfused_golden.py

The reference's `src.upstream.unfused.upstream_expert.Upstream_Expert` is imported, never copied.  Two things are swapped on the
*instance*, as make_goldens.py swaps the dropout: the fc dropout for explicit masks, and the encoder wrapper's `forward`, whose
shipped unpack order (`x, x_1, x_2, x_3 = self.encoder(x)` against an encoder that returns `(x_1, x_2, x_3, x)`) dies in the
classifier - the corrected order below is the original's meaning.  For C = 99 and C = 585: B = 8, T = 96, three SGD
steps, `fill_state_dict_(seed=5)`, labels from `fill.uniform01`.
"""
import copy
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402
from make_goldens import FixedMaskDropout, drop_mask, fill, grad_digest, t2n, views  # noqa: E402

CFG_U = {"pretrain": dict(MG.CFG_M["pretrain"], task_label=99, alpha=0.7, beta=0.3, gamma=0.003)}
for _k in ("contrastive_dim", "lambda_barlow", "loss_scale"):
    CFG_U["pretrain"].pop(_k)
B, T, TP, STEPS = 8, 96, 12, 3


def labels(C, salt):
    return torch.from_numpy(np.floor(fill.uniform01((B,), salt) * C).astype(np.int64))


def corrected_forward(self, x):
    x_1, x_2, x_3, x = self.encoder(x)
    (x1, _) = torch.max(x, dim=1)
    x2 = torch.mean(x, dim=1)
    return x1 + x2, (x_1, x_2, x_3)


def run(XU, ENC, C):
    cfg = copy.deepcopy(CFG_U)
    cfg["pretrain"]["task_label"] = C
    torch.manual_seed(0)
    ex = XU.Upstream_Expert(cfg, base_encoder=ENC.AudioNTT2020Task6)
    fill.fill_state_dict_(ex, seed=5)
    ex.trainer = MG._Trainer()
    fmd = FixedMaskDropout(0.3)
    ex.encoder_q.encoder.fc[2] = fmd
    ex.encoder_q.forward = types.MethodType(corrected_forward, ex.encoder_q)
    logged = []
    ex.log_dict = lambda d, *a, **k: logged.append({k_: float(v.detach()) for k_, v in d.items()})
    ex.train()
    opt = ex.configure_optimizers()
    losses = []
    for s in range(STEPS):
        fmd.masks = [drop_mask((B, TP, 2048), 8100 + s)]
        opt.zero_grad()
        loss = ex.training_step(((views(B, T, 8000 + s), None), labels(C, 8200 + s)), s)
        loss.backward()
        if s == 0:
            gd0 = grad_digest(ex)
        opt.step()
        losses.append(float(loss))
    sd = ex.state_dict()
    terms = np.array([[d["train_loss"], d["CE-loss"], d["kl-loss"], d["mse-loss"]] for d in logged], np.float64)
    tag = f"c{C}_"
    return {tag + "losses": np.array(losses, np.float64), tag + "terms": terms, tag + "g_names": gd0["names"],
            tag + "g_norms": gd0["norms"], tag + "g_heads": gd0["heads"],
            tag + "sd_keys": np.array(list(sd.keys())),
            tag + "sd_shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()]),
            tag + "w_conv1": t2n(sd["encoder_q.encoder.features_1.0.weight"]).ravel(),
            tag + "w_fc2_head": t2n(sd["encoder_q.encoder.fc.3.weight"]).ravel()[:256],
            tag + "w_p1_0_head": t2n(sd["p1.projector.0.weight"]).ravel()[:256],
            tag + "w_p3_6_head": t2n(sd["p3.projector.6.weight"]).ravel()[:256],
            tag + "w_cls_head": t2n(sd["classifier.linear.weight"]).ravel()[:256],
            tag + "b_cls": t2n(sd["classifier.linear.bias"])[:64],
            tag + "bn_rm": t2n(sd["p2.projector.1.running_mean"])[:64]}


def main():
    MG._install_shims()
    sys.path.insert(0, MG.REF)
    importlib.import_module("src.utils.utils")
    ENC = MG._load_by_path("ref_audiontt", os.path.join(MG.REF, "src/encoder/audiontt.py"))
    XU = importlib.import_module("src.upstream.unfused.upstream_expert")
    torch.set_num_threads(8)
    out = {}
    for C in (99, 585):
        out.update(run(XU, ENC, C))
        print(C, out[f"c{C}_losses"])
    MG.save("step_unfused", **out)


if __name__ == "__main__":
    main()
