#!/usr/bin/env python3
"""Audio tagging (multi-label) probe / fine-tuning for both encoder families on the MI355X path.

`train_downstream.py` with several labels per clip: the CSVs have the columns `wav,label` and a label cell holds several names
("dog,bark"; `--label_sep` changes the separator, `--label_csv` maps names through an AudioSet-style `index,mid,display_name`
file, `extras/mast_new/mast/dataloader.py:21-29`).  The target is the multi-hot row of `dataloader.py:157-184`, the loss
nn.BCEWithLogitsLoss (`bce_rows` kernel), the metrics per-class average precision / ROC-AUC / d' of
`extras/mast_new/mast/utilities/stats.py:11-57` (`tagging_stats` kernels): one JSON line per epoch in
`<exp_dir>/<task>/tagging_stats.txt` with epoch, Train_loss, Test_Loss, mAP, mAUC, d_prime, classes_scored, Best_mAP.

  --encoder AudioNTT2020Task6   `DownstreamEncoder(..., no_of_classes=C)` behind the log-mel front end; `--freeze` /
                                `--checkpoint` as in train_downstream.py.  Config: the `run` / `downstream` keys of
                                src/downstream/downstream_config.yaml.
  --encoder ASTModel            `SSMAST(config, emb_dim=C)` (base224 or mvit by `pretrain.base_encoder`): the token mean ->
                                Linear(width, C) the encoder already ends in.  `--checkpoint`: every `encoder_q.*` tensor except
                                `fc.*`; `--freeze` leaves only `fc` trainable.  Kaldi fbank front end (`MastFrontEnd`) with the
                                config's `tagging.freqm / timem / mixup` for training (the targets follow the mix:
                                lam * y + (1 - lam) * y[partner]) and all three at 0 for evaluation.  Config: `run` as above,
                                `pretrain` as src/upstream/ssmast/config.yaml, `tagging` (freqm, timem, mixup, mean, std, skip_norm).

Both paths: the trainable parameters in one flat buffer, one `adamw` launch per step (weight_decay 0 = torch.optim.Adam), one
GPU.  The evaluation pass runs in eval() mode, keeps the logits on the device and hands the RAW logits to one `tagging_stats`
call: they rank at least as finely as their sigmoid (which rounds large logits to 1.0 and would merge them into one tie), and
AP / AUC depend on the ranking alone.
"""
import argparse
import importlib
import json
import os
import sys
import time
from pathlib import Path

import pandas as pd
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from src.dataset.downstream_dataset import DownstreamFrontEnd  # noqa: E402
from src.dataset.upstream_dataset import load_audio  # noqa: E402
from src.evaluation.tagging import (bce_with_logits, build_class_index, mix_labels, multi_hot, parse_labels,  # noqa: E402
                                    tagging_stats)
from src.flat import FlatGroup  # noqa: E402
from src.optim import HipAdamW  # noqa: E402
from src.utils import AverageMeter, extract_window, freeze_encoder, load_pretrained_encoder  # noqa: E402

ENCODERS = ("AudioNTT2020Task6", "ASTModel")
STAT_KEYS = ("epoch", "Train_loss", "Test_Loss", "mAP", "mAUC", "d_prime", "classes_scored", "Best_mAP")


class TaggingDataset(torch.utils.data.Dataset):
    """`wav,label` CSV with several names per label cell -> (window [duration * sr] float32, multi-hot float32 [C])."""

    def __init__(self, csv_path, class_index, duration, sample_rate=16000, sep=","):
        self.dataset = pd.read_csv(csv_path)
        self.class_index = class_index
        self.duration, self.sample_rate = duration, sample_rate
        self.targets = multi_hot([parse_labels(c, sep) for c in self.dataset["label"]], class_index)

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        wave = torch.from_numpy(load_audio(self.dataset["wav"].iloc[idx], self.sample_rate))
        return extract_window(wave, data_size=self.duration), self.targets[idx]


class TaggingTrainer:
    """Model + flat trainable parameters + Adam + BCE-with-logits, with `ProbeTrainer`'s `step` / `train_one_epoch` / `eval`.
    front_end / eval_front_end: waves -> network input; a front end that mixes clips (`MastFrontEnd`) leaves its draws in
    `last_plan` and the train targets follow them (`mix_labels`)."""

    def __init__(self, model, lr, front_end=None, eval_front_end=None):
        self.model = model
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        self.flat = FlatGroup(named)
        model.__dict__.pop("_pd_cache", None)                       # the parameters just moved into the flat buffer
        self.opt = HipAdamW([self.flat], [p for _, p in named], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
        self.front = front_end or DownstreamFrontEnd()
        self.eval_front = eval_front_end or self.front
        self.last_targets = None                                     # the targets of the most recent train batch, after the mix

    def step(self, x, target):
        """One optimisation step on a batch of network inputs and float targets [B, C] in [0, 1] -> loss tensor."""
        flat = self.flat
        flat.zero_grad()
        for p in flat.params:
            p.grad = None
        flat.attach_grads()
        loss = bce_with_logits(self.model(x), target)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def train_targets(self, target, device):
        target = torch.as_tensor(target, dtype=torch.float32).to(device)
        plan = getattr(self.front, "last_plan", None)
        if plan is not None:
            target = mix_labels(target, plan[0], plan[1])
        self.last_targets = target
        return target

    def train_one_epoch(self, loader, epoch, rank=0, log=print):
        losses, batch_time, end = AverageMeter(), AverageMeter(), time.time()
        self.model.train()
        for i, (waves, target) in enumerate(loader):
            x = self.front(waves)
            loss = self.step(x, self.train_targets(target, x.device))
            losses.update(loss, waves.size(0))
            batch_time.update(time.time() - end)
            end = time.time()
            if rank == 0 and log is not None:
                log(f"Epoch: [{epoch}][{i}/{len(loader)}]\tTime: {batch_time.val:.3f} ({batch_time.avg:.3f})\t"
                    f"Loss: {float(losses.val):.4f} ({float(losses.avg):.4f})")
        return dict(epoch=epoch, loss=losses)

    @torch.no_grad()
    def eval(self, loader, epoch=0):
        """-> (stats, logits [N, C], targets [N, C]): `tagging_stats` of the raw logits of the whole split plus `epoch` and
        `loss` (the mean of the per-batch BCE, weighted by batch size); logits and targets stay on the device."""
        self.model.eval()
        losses, logits, targets = AverageMeter(), [], []
        for waves, target in loader:
            x = self.eval_front(waves)
            target = torch.as_tensor(target, dtype=torch.float32).to(x.device)
            out = self.model(x)
            losses.update(bce_with_logits(out, target), waves.size(0))
            logits.append(out.float())
            targets.append(target)
        logits, targets = torch.cat(logits), torch.cat(targets)
        stats = tagging_stats(logits, targets)
        stats.update(epoch=epoch, loss=float(losses.avg))
        return stats, logits, targets


def load_mast_encoder(model, checkpoint):
    """Every `encoder_q.*` tensor of an SS-MAST checkpoint except the embedding head `fc.*` (its width is the pre-training
    embedding's, ours the class count) -> the tagging model.  A tensor the model has and the checkpoint lacks is an error."""
    ck = torch.load(checkpoint, map_location="cpu", weights_only=True)
    sd = ck.get("state_dict", ck)
    pre = "encoder_q."
    wts = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre) and not k[len(pre):].startswith("fc.")}
    missing, unexpected = model.load_state_dict(wts, strict=False)
    missing = [k for k in missing if not k.startswith("fc.")]
    if missing or unexpected:
        raise RuntimeError(f"{checkpoint} does not fit the encoder: missing {missing}, unexpected {list(unexpected)}")
    return model


def build_model(args, config, n_classes):
    """-> (model on the device, train front end, eval front end)."""
    if args.encoder == "ASTModel":
        from src.dataset.mast_dataset import MastFrontEnd
        from src.upstream.ssmast.upstream_encoder import SSMAST
        if "pretrain" not in config:
            raise ValueError("--encoder ASTModel needs a config with the `pretrain` section of src/upstream/ssmast/config.yaml")
        model = SSMAST(config, emb_dim=n_classes)
        if args.checkpoint is not None:
            load_mast_encoder(model, args.checkpoint)
        if args.freeze:
            for n, p in model.named_parameters():
                p.requires_grad = n.startswith("fc.")
        inp, tag = config["pretrain"]["input"], dict(config.get("tagging") or {})
        conf = dict(num_mel_bins=inp["n_mels"], target_length=1 + int(inp["length_wave"] * inp["sampling_rate"]) // 160,
                    freqm=tag.get("freqm", 0), timem=tag.get("timem", 0), mixup=tag.get("mixup", 0.0), mean=tag.get("mean"),
                    std=tag.get("std"), skip_norm=tag.get("skip_norm", tag.get("mean") is None))
        return model.cuda(), MastFrontEnd(conf), MastFrontEnd(dict(conf, freqm=0, timem=0, mixup=0.0))
    base_encoder = getattr(importlib.import_module("src.encoder"), args.encoder)
    config["downstream"]["base_encoder"]["type"] = args.encoder
    from src.downstream.downstream_encoder import DownstreamEncoder
    model = DownstreamEncoder(config, args, base_encoder, no_of_classes=n_classes).cuda()
    if args.freeze:
        freeze_encoder(model)
    if args.checkpoint is not None:
        load_pretrained_encoder(model, args)
    front = DownstreamFrontEnd()
    return model, front, front


def main(args):
    cfg_path = args.config or os.path.join(HERE, "src", "downstream", "downstream_config.yaml")
    with open(cfg_path, "r") as f:
        config = yaml.load(f, Loader=yaml.SafeLoader)
    print(config)
    if int(os.environ.get("WORLD_SIZE", 1)) > 1:
        raise NotImplementedError("train_tagging.py runs on one GPU (more than one rank is out of scope)")
    if not torch.cuda.is_available():
        raise RuntimeError("train_tagging.py (MI355X path) needs a GPU; the HIP kernels have no CPU fallback")
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
    exp_root = Path(args.exp_dir) / args.task
    exp_root.mkdir(parents=True, exist_ok=True)
    run = config["run"]
    class_index = build_class_index(pd.read_csv(args.train_csv)["label"], args.label_csv, args.label_sep)
    n_classes = len(class_index)
    train_dataset = TaggingDataset(args.train_csv, class_index, run["duration"], sep=args.label_sep)
    test_dataset = TaggingDataset(args.test_csv, class_index, run["duration"], sep=args.label_sep)
    train_loader = torch.utils.data.DataLoader(train_dataset, batch_size=run["batch_size"], shuffle=True, pin_memory=True, num_workers=0)
    test_loader = torch.utils.data.DataLoader(test_dataset, batch_size=run["batch_size"], pin_memory=True, num_workers=0)
    model, front, eval_front = build_model(args, config, n_classes)
    trainer = TaggingTrainer(model, run["lr"], front, eval_front)
    trainer.class_index, trainer.test_loader, trainer.last_eval = class_index, test_loader, None
    best, history = float("-inf"), []
    with open(exp_root / "tagging_stats.txt", "a", buffering=1) as stats_file:
        for epoch in range(run["epochs"]):
            train_stats = trainer.train_one_epoch(train_loader, epoch, log=print if args.verbose else None)
            trainer.last_eval = ev, _, _ = trainer.eval(test_loader, epoch)
            if ev["mAP"] == ev["mAP"]:                               # not NaN
                best = max(best, ev["mAP"])
            stats = dict(epoch=epoch, Train_loss=float(train_stats["loss"].avg), Test_Loss=ev["loss"], mAP=ev["mAP"], mAUC=ev["mAUC"],
                         d_prime=ev["d_prime_mean"], classes_scored=ev["classes_scored"],
                         Best_mAP=best if best > float("-inf") else float("nan"))
            print(stats)
            print(json.dumps(stats), file=stats_file)
            history.append(stats)
    print("max valid mAP : {}".format(best))
    return trainer, history


def get_args(argv=None):
    parser = argparse.ArgumentParser(allow_abbrev=False)
    parser.add_argument("--task", type=str, default="test_task")
    parser.add_argument("--train_csv", type=str, required=True)
    parser.add_argument("--valid_csv", type=str, default=None)
    parser.add_argument("--test_csv", type=str, required=True)
    parser.add_argument("--checkpoint", type=str, help="path to pre-trained checkpoint", default=None)
    parser.add_argument("--encoder", type=str, default="AudioNTT2020Task6", choices=ENCODERS)
    parser.add_argument("--freeze", type=lambda s: str(s).lower() not in ("0", "false", "no"), default=True)
    parser.add_argument("--exp_dir", default="./exp", type=Path)
    parser.add_argument("--upstream", type=str, default="delores_m")
    parser.add_argument("-c", "--config", metavar="CONFIG_PATH", default=None)
    parser.add_argument("--verbose", action="store_true")
    parser.add_argument("--label_csv", type=str, default=None, help="index,mid,display_name file mapping label names to columns")
    parser.add_argument("--label_sep", type=str, default=",", help="separator of the names inside a label cell")
    return parser.parse_args(argv)


if __name__ == "__main__":
    main(get_args())
