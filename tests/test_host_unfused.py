"""CPU: the UnFuSeD expert without a GPU - the torch restatement (`tests/unfused_ref.py`) against the reference's own run
(`tests/golden/step_unfused.npz`), the loss kernel's closed-form gradients against fp64 autograd, the padded modules' state_dict,
label validation, the labelled collate and the shipped config."""
import copy
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pcm_cases as P
import unfused_ref as UR
from conftest import CFG_M
from helpers import drop_mask, views
from oracle import fill

CFG_U = {"run": dict(CFG_M["run"], save_path="/tmp/audiossl_u/"),
         "pretrain": dict({k: v for k, v in CFG_M["pretrain"].items() if k not in ("contrastive_dim", "lambda_barlow", "loss_scale")},
                          task_label=99, alpha=0.7, beta=0.3, gamma=0.003)}
B, T, TP = 8, 96, 12


def cfg_u(C, prec=None):
    cfg = copy.deepcopy(CFG_U)
    cfg["pretrain"]["task_label"] = C
    if prec:
        cfg["run"]["precision"] = prec
    return cfg


def golden_labels(C, salt, n=B):
    return torch.from_numpy(np.floor(fill.uniform01((n,), salt) * C).astype(np.int64))


def golden_batches(C, steps=3):
    """The inputs of `make_unfused_golden.py`: (view, labels, dropout keep mask) per step."""
    return [(views(B, T, 8000 + s), golden_labels(C, 8200 + s), drop_mask((B, TP, 2048), 8100 + s)) for s in range(steps)]


def ref_expert(C, seed=5):
    ex = UR.UnfusedExpert(cfg_u(C))
    return fill.fill_state_dict_(ex, seed=seed)


# ------------------------------------------------------------------------------------------------ restatement vs the reference
@pytest.mark.parametrize("C", [99, 585])
def test_restatement_reproduces_the_reference_run(golden, C):
    g = golden("step_unfused")
    torch.set_num_threads(8)
    terms, g0 = UR.run_steps(ref_expert(C), golden_batches(C))
    want = g[f"c{C}_terms"]
    assert np.allclose(g[f"c{C}_losses"], want[:, 0], rtol=1e-7)
    rel = np.abs(terms.numpy() - want) / np.abs(want)
    print("terms rel err", rel.max())
    assert rel.max() <= 1e-5, (terms, want)
    names = list(g[f"c{C}_g_names"])
    assert names == [n for n, _ in ref_expert(C).named_parameters()]
    got = np.array([float(g0[n].norm()) for n in names])
    reln = np.abs(got - g[f"c{C}_g_norms"]) / g[f"c{C}_g_norms"]
    print("grad norm rel err", reln.max())
    assert reln.max() <= 1e-4
    for n, h in zip(names, g[f"c{C}_g_heads"]):
        k = min(8, g0[n].numel())
        assert np.allclose(g0[n].flatten()[:k].numpy(), h[:k], rtol=2e-3, atol=1e-4 * float(g0[n].abs().max()))


# ------------------------------------------------------------------------------------------------ closed-form gradients
def logits64(Bc, C, salt, scale=1.0):
    zs = [torch.from_numpy(fill.normalish((Bc, C), salt + q).astype(np.float64) * scale) for q in range(4)]
    y = golden_labels(C, salt + 9, Bc)
    y[0], y[-1] = 0, C - 1
    return zs, y


@pytest.mark.parametrize("C,scale", [(2, 1.0), (99, 1.0), (99, 8.0), (585, 8.0), (1251, 30.0)])
def test_closed_form_gradients_equal_fp64_autograd(C, scale):
    zs, y = logits64(5, C, 300 + C, scale)
    zs = [z.requires_grad_() for z in zs]
    a, b, g = 0.7, 0.3, 0.003
    total = UR.loss_terms(*zs, y, a, b, g)[0]
    auto = torch.autograd.grad(total, zs)
    closed = UR.closed_form_grads(*[z.detach() for z in zs], y, a, b, g)
    for au, cl in zip(auto, closed):
        assert torch.isfinite(au).all()
        err = float((au - cl).norm() / au.norm())
        print(C, scale, err)
        assert err <= 1e-12


def test_closed_form_gradients_on_zero_rows_take_the_clamp_branch():
    zs, y = logits64(5, 99, 77)
    zs[1][2] = 0
    zs[3][4] = 0
    zs = [z.requires_grad_() for z in zs]
    auto = torch.autograd.grad(UR.loss_terms(*zs, y, 0.7, 0.3, 0.5)[0], zs)
    closed = UR.closed_form_grads(*[z.detach() for z in zs], y, 0.7, 0.3, 0.5)
    for au, cl in zip(auto, closed):
        assert float((au - cl).norm() / au.norm()) <= 1e-12


# ------------------------------------------------------------------------------------------------ state dict of the padded modules
def hip_expert(C, prec=None):
    from src.encoder import AudioNTT2020Task6
    from src.upstream.unfused.upstream_expert import Upstream_Expert
    return Upstream_Expert(cfg_u(C, prec), base_encoder=AudioNTT2020Task6)


HEAD_PREFIXES = ("p1.", "p2.", "p3.", "classifier.")


def padding_of(ex, name, t):
    """The padded part of a head tensor `t` stored under `name` (None when nothing is padded): rows / columns beyond C."""
    C = ex.num_classes
    if not name.startswith(HEAD_PREFIXES) or C % 64 == 0 or t.ndim == 0:
        return None
    parts = [t[C:].flatten()]
    if t.ndim == 2 and t.shape[1] == t.shape[0]:
        parts.append(t[:, C:].flatten())
    return torch.cat(parts)


@pytest.mark.parametrize("C", [99, 585])
def test_state_dict_has_the_reference_keys_and_shapes(golden, C):
    g = golden("step_unfused")
    ex = hip_expert(C)
    sd = ex.state_dict()
    assert list(sd.keys()) == list(g[f"c{C}_sd_keys"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(g[f"c{C}_sd_shapes"])
    assert [n for n, _ in ex.named_parameters()] == list(g[f"c{C}_g_names"])
    # reference-shaped tensors in, the same tensors out, bit for bit; the padding is zero afterwards
    src = {k: v.clone() for k, v in fill.fill_state_dict_(ref_expert(C), seed=9).state_dict().items()}
    for k in src:
        if k.endswith("running_mean"):
            src[k] = torch.from_numpy(fill.uniform(tuple(src[k].shape), 11, -1, 1))
    ex.load_state_dict(src)
    out = ex.state_dict()
    for k, v in src.items():
        assert out[k].shape == v.shape and torch.equal(out[k], v), k
    npad = 0
    for n, p in list(ex.named_parameters()) + list(ex.named_buffers()):
        pad = padding_of(ex, n, p.detach())
        if pad is not None and not n.endswith("running_var"):
            npad += pad.numel()
            assert not pad.any(), n
    assert npad > 0
    assert ex.p1.projector[3].weight.shape == (ex.p1.width, ex.p1.width) and ex.p1.width % 64 == 0


def test_zero_padding_is_a_fixed_point_of_training():
    """The argument of DESIGN.md section 11 in fp64 torch: heads of width C = 99 stored in Cp = 128 with zero padding, the loss
    on the first C columns, 4 SGD steps (momentum, weight decay): the padded model is the plain model and max|pad| stays 0.0."""
    C, Cp, Bc, dims = 99, 128, 8, (48, 32, 16, 48)
    torch.manual_seed(3)
    plain = [UR.Project(d, C).double() for d in dims[:3]] + [UR.Classifier(dims[3], C).double()]
    wide = [UR.Project(d, Cp).double() for d in dims[:3]] + [UR.Classifier(dims[3], Cp).double()]
    with torch.no_grad():
        for a, b in zip(plain, wide):
            for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
                pb.zero_()
                pb[tuple(slice(0, k) for k in pa.shape)] = pa
    params = lambda ms: [p for m in ms for p in m.parameters()]
    opts = [torch.optim.SGD(params(ms), 0.03, momentum=0.9, weight_decay=1e-4) for ms in (plain, wide)]
    for s in range(4):
        xs = [torch.from_numpy(fill.normalish((Bc, d), 60 + 4 * s + i).astype(np.float64)) + 1.5 for i, d in enumerate(dims)]
        y = golden_labels(C, 70 + s, Bc)
        losses = []
        for ms, opt in zip((plain, wide), opts):
            opt.zero_grad()
            loss = UR.loss_terms(*[m.train()(x)[:, :C] for m, x in zip(ms, xs)], y, 0.7, 0.3, 0.003)[0]
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        assert abs(losses[0] - losses[1]) <= 1e-12 * abs(losses[0])
    for a, b in zip(plain, wide):
        for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
            sl = tuple(slice(0, k) for k in pa.shape)
            assert float((pb[sl] - pa).detach().abs().max()) <= 1e-13, n
            rest = pb.detach().clone()
            rest[sl] = 0
            assert float(rest.abs().max()) == 0.0, n
    for b in wide[:3]:
        for i in (1, 4):
            assert float(b.projector[i].running_mean[C:].abs().max()) == 0.0


def test_multiple_of_64_is_not_padded():
    ex = hip_expert(128)
    assert ex.p2.projector[0].weight.shape == (128, 1024) and ex.classifier.linear.bias.shape == (128,)


def test_use_mlp_is_refused():
    from src.encoder import AudioNTT2020Task6
    from src.upstream.unfused.upstream_expert import Upstream_Expert
    with pytest.raises(NotImplementedError):
        Upstream_Expert(cfg_u(99), base_encoder=AudioNTT2020Task6, use_mlp=True)


# ------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("bad", [99, -1])
def test_set_labels_rejects_out_of_range_values_on_the_host(bad):
    ex = hip_expert(99)
    with pytest.raises(ValueError, match=str(bad)):
        ex.set_labels(torch.tensor([0, 5, bad, 98]))
    assert ex._labels is None                                  # nothing was allocated or copied
    key = ex.set_labels(torch.tensor([0, 98, 3]))
    assert ex.set_labels(torch.tensor([1, 2, 3])) == key       # same batch size: same buffer
    assert ex.set_labels(torch.tensor([1, 2, 3, 4])) != key


# ------------------------------------------------------------------------------------------------ C ABI validation (no launch)
EINVAL, EALIGN = -1, -3


def _loss_call(gd=0, z=(4096, 8192, 12288, 16384), label=256, B=5, C=99, ld=128, loss4=512, dz=(20480, 24576, 28672, 32768)):
    """`audiossl_unfused_loss` with fake device addresses: every call here fails a check, so nothing is launched"""
    from src import _native as N
    return N.lib().audiossl_unfused_loss(gd, *z, label, B, C, ld, 0.7, 0.3, 0.003, loss4, *dz, None)


@pytest.mark.parametrize("kw", [dict(z=(None, 8192, 12288, 16384)), dict(z=(4096, 8192, None, 16384)), dict(z=(4096, 8192, 12288, None)),
                                dict(label=None), dict(loss4=None), dict(gd=2), dict(gd=-1), dict(B=0), dict(B=-3), dict(C=1), dict(C=0),
                                dict(C=4097, ld=4100), dict(C=99, ld=96), dict(C=130, ld=128),
                                dict(dz=(None, 24576, 28672, 32768)), dict(dz=(20480, None, None, None)),
                                dict(dz=(20480, 24576, 28672, None)), dict(dz=(None, None, None, 32768))])
def test_loss_kernel_bad_arguments_are_einval(kw):
    assert _loss_call(**kw) == EINVAL


@pytest.mark.parametrize("kw", [dict(ld=126), dict(ld=101), dict(z=(4100, 8192, 12288, 16384)), dict(z=(4096, 8192, 12288, 16392)),
                                dict(dz=(20488, 24576, 28672, 32768)), dict(dz=(20480, 24576, 28672, 32772)),
                                dict(dz=(None, None, None, None), z=(4096, 8200, 12288, 16384))])
def test_loss_kernel_misalignment_is_ealign(kw):
    assert _loss_call(**kw) == EALIGN


# ------------------------------------------------------------------------------------------------ loader
def test_labelled_collate(tmp_path):
    import pandas as pd
    from src.augmentations import AugmentationModule
    from src.dataset import BaseDataset, ingest
    from src.dataset.upstream_dataset import WindowCollate, _CollatedLoader
    cfg = cfg_u(99)
    cfg["pretrain"]["input"]["length_wave"] = 0.25
    unit = 4000
    files = [P.write_clip(tmp_path / f"u{i}.wav", "s16", n, 1, 40 + i) for i, n in enumerate([900, 4000, 5000, 12000, 4001])]
    labels = [7, 0, 98, 3, 3]
    pd.DataFrame({"files": files, "label": labels}).to_csv(tmp_path / "lab.csv", index=False)
    pd.DataFrame({"files": files}).to_csv(tmp_path / "nolab.csv", index=False)
    with pytest.raises(ValueError, match="label"):
        BaseDataset(cfg, SimpleNamespace(upstream="unfused"), str(tmp_path / "nolab.csv"), None)
    outs = {}
    for pcm in (False, True):
        for upstream in ("unfused", "delores_m"):
            ds = BaseDataset(cfg, SimpleNamespace(upstream=upstream), str(tmp_path / "lab.csv"), None, pcm=pcm)
            items = [ds[i] for i in range(5)]
            assert all(isinstance(it, tuple) and isinstance(it[1], int) for it in items) == (upstream == "unfused")
            np.random.seed(4); random.seed(4)
            tf = AugmentationModule(cfg, 10, max_batch=8)
            out = WindowCollate(tf, unit, 64, pcm=pcm)(items)
            outs[pcm, upstream] = out, (random.getstate(), np.random.get_state()[1].copy()), np.array(tf.last_starts)
            if upstream == "unfused":
                assert len(out) == 3 and out[2].dtype == torch.int64 and not out[2].is_cuda and out[2].tolist() == labels
                looped = list(_CollatedLoader([items], WindowCollate(tf, unit, 64, pcm=pcm)))
                assert len(looped) == 1 and len(looped[0]) == 3 and looped[0][2].tolist() == labels
            else:
                assert len(out) == 2
    for pcm in (False, True):
        (a, sa, ta), (b, sb, tb) = outs[pcm, "unfused"], outs[pcm, "delores_m"]
        assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and np.array_equal(ta, tb)          # the random streams, the crops
        wa, wb = (a[0]._host, b[0]._host) if pcm else (a[0], b[0])
        assert isinstance(a[0], ingest.PcmBatch) == pcm and torch.equal(wa, wb)
        assert len(a[1]) == len(b[1])
        for x, y in zip(a[1], b[1]):
            assert (x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y))


def test_shipped_config():
    import train_upstream
    cfg = train_upstream.load_config(SimpleNamespace(config=None, upstream="unfused"))
    pre = cfg["pretrain"]
    assert pre["task_label"] == 99 and all(isinstance(pre[k], float) for k in ("alpha", "beta", "gamma"))
    assert (pre["alpha"], pre["beta"], pre["gamma"]) == (0.7, 0.3, 0.003)
    assert "Kmix" not in pre["augmentations"] and "PatchDrop" not in pre["augmentations"]
    assert cfg["run"]["save_path"] == "src/upstream/unfused" and pre["base_encoder"]["return_all_layers"] is True
