"""UnFuSeD expert on MI355X: one encoder, pseudo-labels, self-distillation from a classifier on the fc output (teacher) into
three `Project` heads on the layer means (students): cross-entropy + KL + normalised MSE.

Same class names, constructor, attributes (`encoder_q`, `p1`..`p3`, `classifier`) and config keys (`task_label`, `alpha`,
`beta`, `gamma`) as `src/upstream/unfused/upstream_expert.py:14-168` of the reference.  `training_step` runs the whole step -
encoder, the three heads, the classifier, the loss (ONE launch: `audiossl_unfused_loss`) and the complete backward - as one
fused sequence of HIP launches (`src.engine`); `loss.backward()` only publishes the gradients.

Any class count: the one-launch BatchNorm kernels need widths that are multiples of 64, so `Project` and `Classifier` own their
parameters and BatchNorm buffers at the padded width Cp = 64 * ceil(C / 64).  The padding is zero and stays exactly zero through
training; `state_dict()` / `load_state_dict()` present and accept the reference's shapes.

Defects of the shipped plug-in: the encoder wrapper's unpack order is corrected, `use_mlp=True`
(touches a non-existent `encoder_k`) raises NotImplementedError, the `validation_step` (undefined names) is omitted.
"""
import torch
import torch.nn as nn

from src import _native as N
from src import engine as E
from src.encoder.audiontt import default_precision
from src.flat import cached_param_dict
from src.functional import LinearFn
from src.module_base import UpstreamModule
from src.upstream.common import EAGER, FusedExpertMixin, FusedStepFn, _world
from src.upstream.unfused.upstream_encoder import UNFUSED as UNFUSED_ENCODER


def padded(C):
    return (C + 63) // 64 * 64


class _Padded:
    """Mixin for a torch layer whose tensors are stored zero-padded: `logical` maps a parameter / buffer name to the shape the
    reference has.  state_dict() shows views of the logical part; load_state_dict() takes logical (or already padded) tensors."""
    logical = {}

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        for name, shape in self.logical.items():
            v = destination.get(prefix + name)
            if v is not None and tuple(v.shape) != tuple(shape):
                destination[prefix + name] = v[tuple(slice(0, s) for s in shape)]

    def _load_from_state_dict(self, state_dict, prefix, *args):
        own = dict(self.named_parameters(recurse=False))
        own.update(dict(self.named_buffers(recurse=False)))
        for name, shape in self.logical.items():
            v = state_dict.get(prefix + name)
            if v is not None and tuple(v.shape) == tuple(shape) and tuple(v.shape) != tuple(own[name].shape):
                full = torch.zeros(own[name].shape, dtype=v.dtype, device=v.device)
                full[tuple(slice(0, s) for s in shape)] = v
                state_dict[prefix + name] = full
        super()._load_from_state_dict(state_dict, prefix, *args)


class _PaddedLinear(_Padded, nn.Linear):
    def __init__(self, in_l, out_l, in_p, out_p, bias):
        ref = nn.Linear(in_l, out_l, bias=bias)          # the reference's default init (and its draws from torch's generator)
        super().__init__(in_p, out_p, bias=bias)
        self.logical = {"weight": (out_l, in_l)}
        with torch.no_grad():
            self.weight.zero_()
            self.weight[:out_l, :in_l] = ref.weight
            if bias:
                self.logical["bias"] = (out_l,)
                self.bias.zero_()
                self.bias[:out_l] = ref.bias


class _PaddedBatchNorm1d(_Padded, nn.BatchNorm1d):
    def __init__(self, c_l, c_p):
        super().__init__(c_p)
        self.logical = {k: (c_l,) for k in ("weight", "bias", "running_mean", "running_var")}
        with torch.no_grad():
            self.weight[c_l:] = 0


class Project(nn.Module):
    """Linear(no bias)-BN-ReLU-Linear(no bias)-BN-ReLU-Linear(no bias), all of width out_dim
    (`src/upstream/unfused/upstream_expert.py:14-26`); parameter container, the arithmetic is `engine.projector_forward /
    projector_backward(final_bn=False)` at the padded width."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        C, Cp = out_dim, padded(out_dim)
        self.out_dim, self.width = C, Cp
        self.projector = nn.Sequential(_PaddedLinear(in_dim, C, in_dim, Cp, False), _PaddedBatchNorm1d(C, Cp), nn.ReLU(inplace=True),
                                       _PaddedLinear(C, C, Cp, Cp, False), _PaddedBatchNorm1d(C, Cp), nn.ReLU(inplace=True),
                                       _PaddedLinear(C, C, Cp, Cp, False))

    def param_dict(self):
        return cached_param_dict(self)

    def forward(self, x):
        raise NotImplementedError("the HIP expert fuses the heads and the loss; call training_step(((img_1, _), label), i)")


class Classifier(nn.Module):
    def __init__(self, in_dim, num_cluster):
        super().__init__()
        self.out_dim, self.width = num_cluster, padded(num_cluster)
        self.linear = _PaddedLinear(in_dim, num_cluster, in_dim, self.width, True)

    def forward(self, x):
        return LinearFn.apply(x, self.linear.weight, self.linear.bias, False)[:, :self.out_dim]


class Upstream_Expert(FusedExpertMixin, UpstreamModule):
    def __init__(self, config, base_encoder, datamodule=None, emb_dim: int = 128, num_negatives: int = 65536,
                 encoder_momentum: float = 0.999, softmax_temperature: float = 0.07, learning_rate: float = 0.03,
                 momentum: float = 0.9, weight_decay: float = 1e-4, data_dir: str = './', batch_size: int = 256,
                 use_mlp: bool = False, num_workers: int = 8, *args, **kwargs):
        super().__init__()
        self.save_hyperparameters()
        if use_mlp:
            raise NotImplementedError("use_mlp is not part of the HIP path")
        self.config = config
        self.base_encoder = base_encoder
        self.datamodule = datamodule
        self.encoder_q = self.init_encoders(self.base_encoder)
        C = int(self.config["pretrain"]["task_label"])
        if not 2 <= C <= 4096:
            raise ValueError(f"pretrain.task_label = {C}: the distillation loss kernel takes 2 .. 4096 classes")
        self.num_classes = C
        self.p1 = Project(2048, C)
        self.p2 = Project(1024, C)
        self.p3 = Project(512, C)
        self.classifier = Classifier(2048, C)
        prec = config.get("run", {}).get("precision")
        self.precision = {"fp32": N.F32, "bf16": N.BF16}.get(prec, default_precision())
        self.encoder_q.encoder.precision = self.precision
        self._labels = None
        self.last_terms = None                # device fp32 [4]: {total, CE, KL, MSE} of the latest step, weighted as logged

    def init_encoders(self, base_encoder):
        return UNFUSED_ENCODER(self.config, base_encoder)

    def forward(self, img_q=None):
        q_raw, (q1, q2, q3) = self.encoder_q(img_q.float().contiguous())
        return q1, q2, q3, self.classifier(q_raw)

    # ------------------------------------------------------------------ labels
    def set_labels(self, labels):
        """The pseudo-labels of the next step -> the expert's int64 device buffer (fixed address: a captured step reads it).
        Checked on the host first; the buffer is re-allocated only when the batch size (or the device) changes, which changes
        `graph_key()` and so triggers a new capture.  Returns the graph key."""
        lab = torch.as_tensor(labels).detach().to("cpu", torch.int64).reshape(-1)
        bad = (lab < 0) | (lab >= self.num_classes)
        if bool(bad.any()):
            raise ValueError(f"label {int(lab[bad][0])} is outside [0, {self.num_classes}) (pretrain.task_label)")
        dev = self.classifier.linear.weight.device
        if self._labels is None or self._labels.shape[0] != lab.shape[0] or self._labels.device != dev:
            self._labels = torch.empty(lab.shape[0], dtype=torch.int64, device=dev)
        self._labels.copy_(lab)
        return self.graph_key()

    def graph_key(self):
        return (None,) if self._labels is None else (self._labels.data_ptr(), self._labels.shape[0])

    # ------------------------------------------------------------------ fused step
    def fused_loss(self, img_1, img_2=None, need_grad=True, runner=None):
        """img_2 is ignored: the reference trains on the first view only (`upstream_expert.py:143-144`)."""
        with E.ARENA.step(img_1.device):          # every zero-initialised scratch of the step: one arena, one clear
            return self._fused_loss(img_1, need_grad, runner)

    def _fused_loss(self, img_1, need_grad, runner):
        """Forward + backward as two collective-free phases (see common.GraphPhases): encoder forward, heads, classifier, loss
        and the heads' backward; then the encoder backward.  The gradient all-reduces start between / after them."""
        R = runner or EAGER
        dt = self.precision
        E.set_high_precision(False)
        if E.SYNC_BN is not None:
            raise NotImplementedError("run.sync_batchnorm is not supported by the unfused expert (the reference harness does not "
                                      "convert it)")
        enc = self.encoder_q.encoder
        flat = self.ensure_flat()
        dev = img_1.device
        B = img_1.shape[0]
        C, Cp = self.num_classes, self.classifier.width
        labels = self._labels
        if labels is None or labels.shape[0] != B or labels.device != dev:
            raise RuntimeError(f"set_labels() has not been called for this batch (batch of {B}, labels "
                               f"{None if labels is None else tuple(labels.shape)})")
        pre = self.config["pretrain"]
        alpha, beta, gamma = float(pre["alpha"]), float(pre["beta"]), float(pre["gamma"])
        heads = (self.p1, self.p2, self.p3)
        G = flat.grad_dict
        td = N.torch_dtype(dt)

        def forward_phase():
            if need_grad:
                flat.zero_grad()
            flat.refresh_shadow(dt)
            img = img_1.float().contiguous()
            P = enc.param_dict()
            Wenc = flat.shadow_dict("encoder_q.encoder.")
            Xs = tuple(torch.empty(B, f, dtype=E.pooled_dtype(dt), device=dev) for f in (2048, 1024, 512))
            keep = enc.next_keep_mask(B, img.shape[-1])
            _, _, _, H, c = E.encoder_forward(P, img, dt, keep=keep, p_drop=enc.fc[2].p, train=self.training, Wc=Wenc,
                                              layer_out=Xs)
            # teacher: classifier on max + mean over time of the fc output
            y, arg = E.maxmean_forward(dt, H)
            wc = flat.shadow_dict("classifier.")["linear.weight"]
            t = E.linear_fwd(dt, y, wc, B, Cp, wc.shape[1], bias=self.classifier.linear.bias.data, out_f32=1)
            # students: the three Project chains on the layer means, fp32 logits
            zs, ctxs = [], []
            for i, p in enumerate(heads):
                Wp = flat.shadow_dict(f"p{i + 1}.")
                z, pc = E.projector_forward(p.param_dict(), Xs[i], dt, 1, B, update_running=self.training,
                                            Wc=tuple(Wp[f"projector.{j}.weight"] for j in (0, 3, 6)), final_bn=False)
                zs.append(z)
                ctxs.append(pc)
            loss4 = E.ARENA.zeros((4,), torch.float32, device=dev)
            dz = [torch.empty(B, Cp, dtype=td, device=dev) for _ in range(4)] if need_grad else [None] * 4
            N.call("unfused_loss", dt, zs[0], zs[1], zs[2], t, labels, B, C, Cp, alpha, beta, gamma, loss4, *dz)
            terms = loss4.clone()                   # the arena is cleared by the next step
            if not need_grad:
                return terms, c, None, None
            dxs = [E.projector_backward(pc, p.param_dict(), G(f"p{i + 1}."), dz[i])
                   for i, (p, pc) in enumerate(zip(heads, ctxs))]
            Gc = G("classifier.")
            E.linear_bwd_w(dt, dz[3], y, Gc["linear.weight"], B, Cp, wc.shape[1])
            E.colsum_add(dt, dz[3], B, Cp, Gc["linear.bias"])
            dy = E.linear_bwd_x(dt, dz[3], wc, B, Cp, wc.shape[1], out_f32=1)
            dA2 = E.maxmean_backward(dt, dy, arg, H)
            return terms, c, dA2, dxs
        terms, c, dA2, dxs = R.phase("forward", forward_phase)
        if need_grad:
            self.reduce_begin("heads")                      # p1..p3 and classifier gradients are complete

            def backward_phase():
                E.encoder_backward(c, G("encoder_q.encoder."), dA2=dA2, dx1=dxs[0], dx2=dxs[1], dx3=dxs[2])
            R.phase("encoder_bwd", backward_phase)
            self.reduce_begin("enc")
        self.last_terms = terms
        return terms[0]

    def graph_phases_supported(self):
        return E.SYNC_BN is None

    def training_step(self, batch, batch_idx):
        (img_1, _), label = batch
        cfg_run = self.config.get("run", {})
        if cfg_run.get("sync_batchnorm", False) and _world() > 1:
            raise NotImplementedError("run.sync_batchnorm is not supported by the unfused expert (the reference harness does not "
                                      "convert it)")
        self.set_labels(label)
        params = self.ensure_flat().params
        loss = FusedStepFn.apply(self, torch.is_grad_enabled(), img_1, img_1, *params)
        t = self.last_terms
        self.log_dict({'train_loss': loss, 'kl-loss': t[2], 'CE-loss': t[1], 'mse-loss': t[3]})
        return loss
