"""Torch-CPU restatement of the UnFuSeD expert (`src/upstream/unfused/upstream_expert.py:14-36, 109-168` and
`src/utils/utils.py:191-197` of the reference, with the encoder wrapper's unpack order corrected as DESIGN.md records):
the module tree and state_dict keys of the reference, the loss in any floating dtype, and the closed-form gradients of the
loss kernel (`audiossl_unfused_loss`) written out for comparison with autograd."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import model as OM


class Project(nn.Module):
    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.projector = nn.Sequential(nn.Linear(in_dim, out_dim, bias=False), nn.BatchNorm1d(out_dim), nn.ReLU(inplace=True),
                                       nn.Linear(out_dim, out_dim, bias=False), nn.BatchNorm1d(out_dim), nn.ReLU(inplace=True),
                                       nn.Linear(out_dim, out_dim, bias=False))

    def forward(self, x):
        return self.projector(x)


class Classifier(nn.Module):
    def __init__(self, in_dim, num_cluster):
        super().__init__()
        self.linear = nn.Linear(in_dim, num_cluster)

    def forward(self, x):
        return self.linear(x)


class UNFUSED(nn.Module):
    def __init__(self, config):
        super().__init__()
        be = config["pretrain"]["base_encoder"]
        self.encoder = OM.AudioNTT2020Task6(config["pretrain"]["input"]["n_mels"], be["output_dim"], True)

    def forward(self, x, drop_mask=None):
        x_1, x_2, x_3, x = self.encoder(x, drop_mask)          # the encoder's own order: layer means first, fc output last
        return x.max(dim=1).values + x.mean(dim=1), (x_1, x_2, x_3)


def loss_terms(z1, z2, z3, t, y, alpha, beta, gamma):
    """-> (total, CE, KL, MSE) as the reference logs them (the KL target soft-max is NOT detached)."""
    zs = (z1, z2, z3)
    ce = alpha * sum(F.cross_entropy(z, y) for z in zs) + F.cross_entropy(t, y)
    targets = F.softmax(t, dim=1)
    kl = beta * sum(F.kl_div(F.log_softmax(z, dim=1), targets, reduction="batchmean") for z in zs)

    def mse(a, b):
        return (2 - 2 * (F.normalize(a, dim=-1, p=2) * F.normalize(b, dim=-1, p=2)).sum(dim=-1)).mean()
    ms = gamma * sum(mse(z, t) for z in zs)
    return ms + kl + ce, ce, kl, ms


def closed_form_grads(z1, z2, z3, t, y, alpha, beta, gamma, eps=1e-12):
    """The gradient formulas the loss kernel implements -> (dz1, dz2, dz3, dt).  A norm below eps takes the clamp's autograd:
    the projection term vanishes and the divisor is eps."""
    B, C = t.shape
    oh = F.one_hot(y, C).to(t.dtype)
    lpt = t - torch.logsumexp(t, dim=1, keepdim=True)
    pt = lpt.exp()
    nt = t.norm(dim=1, keepdim=True)
    ntc = nt.clamp_min(eps)
    th = t / ntc
    live_t = (nt >= eps).to(t.dtype)
    dt = (pt - oh) / B
    dzs = []
    for z in (z1, z2, z3):
        lps = z - torch.logsumexp(z, dim=1, keepdim=True)
        ps = lps.exp()
        nz = z.norm(dim=1, keepdim=True)
        nzc = nz.clamp_min(eps)
        zh = z / nzc
        live_z = (nz >= eps).to(t.dtype)
        cos = (zh * th).sum(dim=1, keepdim=True)
        klrow = (pt * (lpt - lps)).sum(dim=1, keepdim=True)
        dzs.append((alpha * (ps - oh) + beta * (ps - pt)) / B - (2 * gamma / B) * (th - live_z * cos * zh) / nzc)
        dt = dt + (beta / B) * pt * ((lpt - lps) - klrow) - (2 * gamma / B) * (zh - live_t * cos * th) / ntc
    return dzs[0], dzs[1], dzs[2], dt


class UnfusedExpert(nn.Module):
    """Reference-keyed module tree: encoder_q.encoder.*, p1..p3.projector.*, classifier.linear.*"""

    def __init__(self, config, learning_rate=0.03, momentum=0.9, weight_decay=1e-4):
        super().__init__()
        self.config = config
        self.hyper = (learning_rate, momentum, weight_decay)
        C = config["pretrain"]["task_label"]
        self.encoder_q = UNFUSED(config)
        self.p1, self.p2, self.p3 = Project(2048, C), Project(1024, C), Project(512, C)
        self.classifier = Classifier(2048, C)

    def logits(self, img, drop_mask=None):
        q_raw, (q1, q2, q3) = self.encoder_q(img, drop_mask)
        return self.p1(q1), self.p2(q2), self.p3(q3), self.classifier(q_raw)

    def training_terms(self, img, label, drop_mask=None):
        p = self.config["pretrain"]
        return loss_terms(*self.logits(img, drop_mask), label.long(), p["alpha"], p["beta"], p["gamma"])

    def configure_optimizers(self):
        lr, mom, wd = self.hyper
        return torch.optim.SGD(self.parameters(), lr, momentum=mom, weight_decay=wd)


def run_steps(expert, batches):
    """batches: [(img, label, drop_mask)] -> (terms [steps, 4] float64 = total / CE / KL / MSE, gradients of step 0 by name)."""
    expert.train()
    opt = expert.configure_optimizers()
    terms, g0 = [], None
    for s, (img, label, mask) in enumerate(batches):
        opt.zero_grad()
        tt = expert.training_terms(img, label, mask)
        tt[0].backward()
        if s == 0:
            g0 = {n: p.grad.detach().clone() for n, p in expert.named_parameters()}
        opt.step()
        terms.append([float(v.detach()) for v in tt])
    return torch.tensor(terms, dtype=torch.float64), g0
