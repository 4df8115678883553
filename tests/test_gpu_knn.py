"""k-NN evaluation on the GPU: `audiossl_knn_topk` / `audiossl_knn_vote` against the int64 / fp64 restatements of
`tests/knn_ref.py`, the Python layer above them, embeddings out of the encoders against the oracle, and the two commands."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import knn_ref as R
from helpers import rel_l2
from oracle import fill

pytestmark = pytest.mark.gpu

GUARD = 2


def _launch_topk(q, bank, k):
    """The C entry on buffers with two guard rows of a recognisable pattern behind them -> (top_sim, top_idx) on the CPU."""
    from src import _native as N
    from src.evaluation.knn import workspace_bytes
    nq, d = q.shape
    nb = bank.shape[0]
    sim = torch.empty(nq + GUARD, k, dtype=torch.float32)
    idx = torch.empty(nq + GUARD, k, dtype=torch.int32)
    sim[:nq] = float("nan")
    idx[:nq] = -5
    sim[nq:] = torch.arange(GUARD * k, dtype=torch.float32).view(GUARD, k) + 1000.5
    idx[nq:] = -(torch.arange(GUARD * k, dtype=torch.int32).view(GUARD, k) + 77)
    sim_d, idx_d = sim.cuda(), idx.cuda()
    nbytes = workspace_bytes(nq, nb, k)
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")          # the kernel clears what it needs itself
    qd, bd = q.cuda(), bank.cuda()
    N.call("knn_topk", qd, bd, nq, nb, d, k, sim_d, idx_d, ws, nbytes)
    torch.cuda.synchronize()
    assert torch.equal(sim_d[nq:].cpu(), sim[nq:]) and torch.equal(idx_d[nq:].cpu(), idx[nq:]), "guard rows overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "workspace overrun"
    assert torch.equal(qd.cpu(), q) and torch.equal(bd.cpu(), bank)
    return sim_d[:nq].cpu(), idx_d[:nq].cpu()


def _ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=g)


# ---- 1. exact cases, ties included -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nb,d,k", [(1, 128, 32, 128), (63, 1000, 256, 128), (130, 70001, 64, 20), (64, 4096, 2048, 1),
                                       (5, 20, 96, 20),
                                       (70, 1100, 32, 64),     # one-slot list, every lane in use; 2 splits: the merge runs
                                       (70, 1100, 32, 65),     # two-slot list, k-th entry = lane 0 of slot 1: every insertion carries
                                       (3, 130, 32, 65)])      # two-slot list, one split, second bank tile with 2 valid rows
def test_topk_exact_on_integer_inputs_ties_by_ascending_row(nq, nb, d, k):
    """Entries in -2..2 are exact in bf16 and every dot product is an integer below 2^24: exact in fp32 in any summation order.
    About 110-160 distinct values per row, so at Nb = 70,001 almost every returned position sits inside a tie: this pins the
    order.  top_sim and top_idx must be EQUAL to the int64 reference."""
    q, bank = _ints((nq, d), 11 + nq), _ints((nb, d), 13 + nb)
    want_d, want_i = R.topk_exact_int(q, bank, k)
    if nb >= 1000:
        assert int((want_d[:, 1:] == want_d[:, :-1]).sum()) > 0 or k == 1          # the case does contain ties
    sim, idx = _launch_topk(q.to(torch.bfloat16), bank.to(torch.bfloat16), k)
    assert torch.equal(idx.to(torch.int64), want_i)
    assert torch.equal(sim.double(), want_d.double())


# ---- 2. real-valued cases ------------------------------------------------------------------------------------------------
def _unit_rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)


def _check_real(sim, idx, ref, k, atol):
    """The rules of the real-valued cases, for EVERY row: (a) descending, distinct, in range; (b) each returned similarity is its
    row's fp64 dot product within atol; (c) the returned values are the reference's top-k values within atol; (d) no returned
    row lies more than 2 atol below the reference's k-th value."""
    nq, nb = ref.shape
    idx = idx.to(torch.int64)
    sim = sim.double()
    assert bool(torch.isfinite(sim).all())
    assert bool((sim[:, 1:] <= sim[:, :-1]).all()), "not descending"
    assert bool(((idx >= 0) & (idx < nb)).all()), "index out of range"
    assert all(len(set(r)) == k for r in idx.tolist()), "duplicate neighbour"
    at = ref.gather(1, idx)
    err_b = float((sim - at).abs().max())
    top = ref.topk(k, dim=1).values
    err_c = float((sim - top).abs().max())
    slack_d = float((top[:, -1:] - at).max())
    print(f"knn real-valued: |sim - ref[idx]| {err_b:.3e}, |sim - ref topk| {err_c:.3e}, kth - ref[idx] {slack_d:.3e}, atol {atol:.3e}")
    assert err_b <= atol
    assert err_c <= atol
    assert slack_d <= 2 * atol


@pytest.mark.parametrize("nq,nb,d,k", [(64, 4096, 2048, 20), (130, 70001, 96, 20), (33, 1000, 768, 128)])
def test_topk_real_valued_within_the_fp32_accumulation_bound(nq, nb, d, k):
    """Unit-norm Gaussian rows rounded to bf16 against fp64 dot products of the rounded values.  atol = D 2^-24: the worst-case
    fp32 accumulation error of D products with sum |q_i b_i| <= 1 (derived, not measured)."""
    q, bank = _unit_rows(nq, d, 3), _unit_rows(nb, d, 4)
    sim, idx = _launch_topk(q, bank, k)
    _check_real(sim, idx, R.sims_f64(q, bank), k, d * 2.0 ** -24)


# ---- 3. planted neighbours -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [768, 2048])
def test_topk_planted_neighbours_indices_exact(d):
    """Each query's 20 true neighbours sit at cosines 0.95, 0.93, ... (0.02 apart, the rest of the bank far below): the
    reference's own gaps are asserted to exceed 0.01, far above atol, so the indices must equal the reference's."""
    nq, k, extra = 40, 20, 1500
    g = torch.Generator().manual_seed(d)
    q = torch.randn(nq, d, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    rows = []
    for i in range(nq):
        n = torch.randn(k, d, generator=g, dtype=torch.float64)
        n = n - (n @ q[i])[:, None] * q[i][None, :]
        n = n / n.norm(dim=1, keepdim=True)
        c = 0.95 - 0.02 * torch.arange(k, dtype=torch.float64)
        rows.append(c[:, None] * q[i][None, :] + (1 - c * c).sqrt()[:, None] * n)
    noise = torch.randn(extra, d, generator=g, dtype=torch.float64)
    bank = torch.cat(rows + [noise / noise.norm(dim=1, keepdim=True)])
    bank = bank[torch.randperm(bank.shape[0], generator=g)]
    qb, bb = q.to(torch.bfloat16), bank.to(torch.bfloat16)
    ref = R.sims_f64(qb, bb)
    top = ref.topk(k + 1, dim=1)
    assert float((top.values[:, :-1] - top.values[:, 1:]).min()) >= 0.01
    sim, idx = _launch_topk(qb, bb, k)
    assert torch.equal(idx.to(torch.int64), top.indices[:, :k])
    assert float((sim.double() - top.values[:, :k]).abs().max()) <= d * 2.0 ** -24


# ---- 4. footprint ----------------------------------------------------------------------------------------------------------
def test_topk_never_materialises_the_similarity_matrix():
    """Nq = 256 against Nb = 262,144: the fp32 matrix would be 256 MiB; outputs + workspace must stay within 32 MiB of torch's
    allocator (every byte of scratch goes through it), and the results are exact."""
    from src.evaluation.knn import knn_topk_bf16
    nq, nb, d, k = 256, 262144, 64, 20
    q, bank = _ints((nq, d), 5), _ints((nb, d), 6)
    want_d, want_i = R.topk_exact_int(q, bank, k)
    qd, bd = q.to(torch.bfloat16).cuda(), bank.to(torch.bfloat16).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    sim, idx = knn_topk_bf16(qd, bd, k)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f"knn footprint: peak growth {growth / 2 ** 20:.2f} MiB (matrix: {nq * nb * 4 / 2 ** 20:.0f} MiB)")
    assert growth <= 32 * 2 ** 20
    assert torch.equal(idx.cpu().to(torch.int64), want_i)
    assert torch.equal(sim.cpu().double(), want_d.double())


# ---- 5. vote ---------------------------------------------------------------------------------------------------------------
BIG = 1 << 40


def test_vote_majority_and_ties_go_to_the_smaller_label():
    from src.evaluation.knn import knn_predict
    labels = torch.tensor([4, 4, 4, 9, 9, 9, 2, 2, 2, -BIG, -BIG, BIG, BIG, 7], dtype=torch.int64)     # bank rows 0..13
    idx = torch.tensor([[0, 3, 1, 6, 2, 4],         # 4 4 4 9 9 2            -> 4 (3 of 6)
                        [3, 0, 4, 1, 6, 13],        # 9 4 9 4 2 7            -> two-way tie 4 | 9 -> 4
                        [6, 3, 0, 7, 4, 1],         # 2 9 4 2 9 4            -> three-way tie -> 2
                        [11, 9, 12, 10, 13, 0],     # +2^40 -2^40 +2^40 -2^40 7 4 -> tie of the far labels -> -2^40
                        [11, 12, 9, 0, 3, 6],       # +2^40 twice             -> +2^40
                        [13, 13, 13, 0, 0, 3]],     # a repeated row still counts per neighbour -> 7
                       dtype=torch.int32)
    sim = torch.linspace(0.9, 0.1, 6).repeat(6, 1)
    pred, conf = knn_predict(sim.cuda(), idx.cuda(), labels.cuda(), temperature=None)
    assert pred.cpu().tolist() == [4, 4, 2, -BIG, BIG, 7]
    np.testing.assert_allclose(conf.cpu().numpy(), [3 / 6, 2 / 6, 2 / 6, 2 / 6, 2 / 6, 3 / 6], rtol=1e-6)
    want, wconf, _ = R.vote(sim, idx, labels, 0.0)
    assert torch.equal(pred.cpu(), want)
    # k = 128 of one label each but two: every lane and both halves take part
    idx = torch.arange(128, dtype=torch.int32)[None, :].repeat(2, 1)
    labels = torch.arange(128, dtype=torch.int64) * 3 - 50
    labels[100] = labels[127]
    pred, conf = knn_predict(torch.zeros(2, 128).cuda(), idx.cuda(), labels.cuda(), temperature=None)
    assert pred.cpu().tolist() == [int(labels[127])] * 2 and float(conf[0]) == pytest.approx(2 / 128)


def test_vote_weighted_matches_fp64_and_out_of_range_rows_are_flagged():
    from src.evaluation.knn import knn_predict
    nq, k, nb, T = 64, 20, 500, 0.07
    g = torch.Generator().manual_seed(12)
    sim = (0.2 + 0.7 * torch.rand(nq, k, generator=g)).sort(dim=1, descending=True).values
    idx = torch.stack([torch.randperm(nb, generator=g)[:k] for _ in range(nq)]).to(torch.int32)
    labels = torch.randint(0, 5, (nb,), generator=g) * 1000 - 2000
    want, wconf, sums = R.vote(sim, idx, labels, 1.0 / T)
    for r, s in enumerate(sums):                         # the comparison is only meaningful where the winner is clear: every row is
        assert len(s) == 1 or (s[0] - s[1]) > 1e-4 * s[0], r
    pred, conf = knn_predict(sim.cuda(), idx.cuda(), labels.cuda(), temperature=T)
    assert torch.equal(pred.cpu(), want)
    assert float((conf.cpu().double() - wconf).abs().max()) <= 1e-5
    bad = idx.clone()
    bad[3, 7] = nb
    bad[9, 0] = -1
    pred, conf = knn_predict(sim.cuda(), bad.cuda(), labels.cuda(), temperature=T)
    pred, conf = pred.cpu(), conf.cpu()
    assert pred[3].item() == -1 and pred[9].item() == -1 and torch.isnan(conf[3]) and torch.isnan(conf[9])
    keep = [r for r in range(nq) if r not in (3, 9)]
    assert torch.equal(pred[keep], want[keep]) and bool(torch.isfinite(conf[keep]).all())


# ---- 6. wrapper --------------------------------------------------------------------------------------------------------------
def test_wrapper_normalises_pads_and_slabs():
    from src.evaluation.knn import knn_topk, normalize_bf16
    nq, nb, d, k = 45, 3000, 100, 20
    g = torch.Generator().manual_seed(8)
    q = torch.randn(nq, d, generator=g) * 3.0
    bank = torch.randn(nb, d, generator=g) * 0.5 + 0.1
    qn, bn = normalize_bf16(q.cuda()).cpu(), normalize_bf16(bank.cuda()).cpu()
    assert qn.shape == (nq, 128) and qn.dtype == torch.bfloat16 and bool((qn[:, d:] == 0).all()) and bool((bn[:, d:] == 0).all())
    assert float((qn[:, :d].float() - torch.nn.functional.normalize(q, dim=1)).abs().max()) <= 2.0 ** -8
    sim, idx = knn_topk(q.cuda(), bank.cuda(), k)
    assert sim.shape == (nq, k) and idx.shape == (nq, k)
    _check_real(sim.cpu(), idx.cpu(), R.sims_f64(qn, bn), k, 128 * 2.0 ** -24)
    sim7, idx7 = knn_topk(q.cuda(), bank.cuda(), k, slab=7)
    assert torch.equal(sim7, sim) and torch.equal(idx7, idx)
    sim_b, idx_b = knn_topk(q.cuda().to(torch.bfloat16), bank.cuda(), k)              # bf16 input is accepted
    assert sim_b.shape == (nq, k)


# ---- 7. embeddings -------------------------------------------------------------------------------------------------------
def _write_wavs(tmp_path, lengths, salt=900):
    from scipy.io import wavfile
    files, waves = [], []
    for i, L in enumerate(lengths):
        w = fill.uniform((L,), salt + i, -0.3, 0.3) + 0.2 * np.sin(2 * np.pi * (200 + 40 * i) * np.arange(L) / 16000).astype(np.float32)
        pcm = (w * 32767).astype(np.int16)
        p = str(tmp_path / f"emb{salt}_{i}.wav")
        wavfile.write(p, 16000, pcm)
        files.append(p)
        waves.append(torch.from_numpy(pcm.astype(np.float32) / 32768.0))
    return files, waves


def _center(w, unit=16000):
    n = len(w)
    if n >= unit:
        s = (n - unit) // 2
        return w[s:s + unit]
    out = torch.zeros(unit)
    left = (unit - n) // 2
    out[left:left + n] = w
    return out


def _nontrivial_bn_(m, seed):
    with torch.no_grad():
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(torch.from_numpy(fill.uniform(tuple(b.shape), seed + fill.salt_of(n) % 1000, -0.2, 0.2)))
            elif n.endswith("running_var"):
                b.copy_(torch.from_numpy(fill.uniform(tuple(b.shape), seed + 1 + fill.salt_of(n) % 1000, 0.5, 1.5)))


def test_embeddings_of_the_conv_encoder_vs_oracle_in_eval_mode(tmp_path, cfg_s):
    from oracle import frontend as FE
    from oracle import model as OM
    from src.encoder import AudioNTT2020Task6
    from src.evaluation import Embedder, extract_embeddings
    from src.upstream.delores_s.upstream_expert import Upstream_Expert
    files, waves = _write_wavs(tmp_path, (9000, 16000, 20000, 23001))
    ref = OM.AudioNTT2020Task6(64, 2048, False)
    fill.fill_state_dict_(ref, seed=21)
    _nontrivial_bn_(ref, 500)
    ref.eval()
    with torch.no_grad():
        x = FE.log_mel_batch(torch.stack([_center(w) for w in waves])).unsqueeze(1)
        h = ref(x)
        want = {"backbone": h.mean(1), "head": h.max(1).values + h.mean(1)}
    cfg = copy.deepcopy(cfg_s)
    expert = Upstream_Expert(cfg, base_encoder=AudioNTT2020Task6)
    expert.encoder.encoder.load_state_dict(ref.state_dict())
    expert = expert.cuda().train()
    flags = [m.training for m in expert.modules()]
    before = {k: v.clone() for k, v in expert.state_dict().items()}
    for layer in ("backbone", "head"):
        for prec, bar in (("fp32", 1e-4), ("bf16", 2e-2)):
            emb = Embedder(expert, layer=layer, precision=prec)
            got = extract_embeddings(emb, files, batch_size=3, window="center", duration=1.0)     # 3 + a final short batch of 1
            assert got.shape == (4, 2048) and got.dtype == torch.float32 and got.is_cuda
            e = rel_l2(got.cpu(), want[layer])
            print(f"embeddings {layer} {prec}: rel-L2 {e:.3e} (bar {bar})")
            assert e <= bar, (layer, prec, e)
            again = extract_embeddings(emb, files, batch_size=3, window="center", duration=1.0)
            assert torch.equal(again, got)
    assert [m.training for m in expert.modules()] == flags
    after = expert.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    # the bare encoder, the packed-PCM path and the random window
    bare = Embedder(expert.encoder.encoder, layer="backbone", precision="fp32")
    got = extract_embeddings(bare, files, batch_size=4)
    assert rel_l2(got.cpu(), want["backbone"]) <= 1e-4
    got_pcm = extract_embeddings(bare, files, batch_size=4, pcm=True)
    assert torch.equal(got_pcm, got)
    import random
    random.seed(3)
    r1 = extract_embeddings(bare, files, batch_size=4, window="random")
    assert r1.shape == (4, 2048) and torch.equal(r1[:2], got[:2]) and not torch.equal(r1[2:], got[2:])


def _t(shape, salt, lo, hi):
    return torch.from_numpy(fill.uniform(shape, salt, lo, hi))


def test_embeddings_of_the_ast_encoder_vs_oracle(tmp_path):
    """base224, depth 2: backbone = the oracle's token mean (the input of its `fc`) at the bar test_gpu_vit.py holds the encoder
    output to; head = the module's own forward, bit for bit."""
    from helpers import views
    from oracle import vit as OV
    from src.encoder import ASTModel
    from src.evaluation import Embedder, extract_embeddings
    B, F_, T = 4, 128, 101
    kw = dict(label_dim=256, fstride=10, tstride=10, input_fdim=F_, input_tdim=T, depth=2)
    ref = OV.ASTModel(**kw)
    fill.fill_state_dict_(ref, seed=42)
    with torch.no_grad():
        ref.v.pos_embed.copy_(_t(tuple(ref.v.pos_embed.shape), 41, -0.05, 0.05))
    m = ASTModel(**kw)
    m.load_state_dict(ref.state_dict())
    m = m.cuda().train()
    x = torch.cat([views(B, T, 700 + i) for i in range(2)], dim=2).contiguous()
    seen = []
    hook = ref.fc.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].detach()))
    with torch.no_grad():
        ref(x)
    hook.remove()
    back = Embedder(m, layer="backbone")(x.cuda())
    assert back.shape == (B, 768) and back.dtype == torch.float32
    assert rel_l2(back.cpu(), seen[0]) < 2e-2
    head = Embedder(m, layer="head")(x.cuda())
    with torch.no_grad():
        own = m(x.cuda())
    assert torch.equal(head, own) and m.training
    # through the files: the fbank front end with masking and mixing off, an odd final batch
    files, _ = _write_wavs(tmp_path, (9000, 16000, 20000), salt=950)
    emb = Embedder(m, layer="backbone", input_shape=(F_, T))
    e1 = extract_embeddings(emb, files, batch_size=2)
    e2 = extract_embeddings(emb, files, batch_size=2)
    assert e1.shape == (3, 768) and bool(torch.isfinite(e1).all()) and torch.equal(e1, e2)


def test_embeddings_of_the_mvit_encoder_vs_oracle():
    """mvit, the shallow layout of test_gpu_vit.py: backbone against `oracle.mvit.mvit_encoder` with an identity `fc` (its output
    is then the token mean, exactly); head = the module's own forward, bit for bit."""
    from helpers import views
    from oracle import mvit as OM
    from src.encoder import ASTModel
    from src.evaluation import Embedder
    B, F_, T, depth = 2, 128, 301, 6
    mv = dict(depth=depth, dim_mul=((1, 2.0), (3, 2.0)), head_mul=((1, 2.0), (3, 2.0)), q_strides=((1, 2, 2), (3, 2, 2)),
              kv_stride_adaptive=(4, 4))
    m = ASTModel(label_dim=256, input_fdim=F_, input_tdim=T, model_size="mvit", mvit=mv)
    fill.fill_state_dict_(m, seed=60 + depth)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "rel_pos" in n:
                p.copy_(_t(tuple(p.shape), fill.salt_of(n), -0.2, 0.2))
    P = {n: p.detach().clone() for n, p in m.named_parameters()}
    width = P["fc.weight"].shape[1]
    P["fc.weight"], P["fc.bias"] = torch.eye(width), torch.zeros(width)
    blocks = [dict(dim=c.dim, dim_out=c.dim_out, heads=c.heads, hw=c.hw, stride_q=c.stride_q, stride_kv=c.stride_kv, rel_pos=c.rel_pos,
                   residual_pooling=c.residual_pooling, dim_mul_in_att=c.dim_mul_in_att) for c in m.cfg["blocks"]]
    x = torch.cat([views(B, T, 720 + i) for i in range(2)], dim=2).contiguous()
    with torch.no_grad():
        want = OM.mvit_encoder(P, x, blocks)
    m = m.cuda().eval()
    back = Embedder(m, layer="backbone")(x.cuda())
    assert back.shape == (B, width)
    assert rel_l2(back.cpu(), want) < 2e-2
    head = Embedder(m, layer="head")(x.cuda())
    with torch.no_grad():
        own = m(x.cuda())
    assert torch.equal(head, own) and not m.training


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------
def test_knn_classifier_on_planted_clusters():
    from src.evaluation import KnnClassifier
    g = torch.Generator().manual_seed(1)
    centres = torch.eye(3, 48) * 4.0
    y_bank = torch.arange(60) % 3
    y_q = torch.arange(30) % 3
    bank = centres[y_bank] + 0.1 * torch.randn(60, 48, generator=g)
    q = centres[y_q] + 0.1 * torch.randn(30, 48, generator=g)
    ids = torch.tensor([10, -3, 1 << 35])                  # labels are values, not indices
    clf = KnnClassifier(k=20, temperature=0.07).fit(bank.cuda(), ids[y_bank].cuda())
    assert clf.score(q.cuda(), ids[y_q].cuda()) == 1.0
    pred, conf = clf.predict(q.cuda(), return_conf=True)
    assert torch.equal(pred.cpu(), ids[y_q]) and float(conf.min()) > 0.99
    with pytest.raises(ValueError):
        KnnClassifier(k=20).fit(bank[:10].cuda(), y_bank[:10])


def _checkpoint(tmp_path, cfg_s):
    from src.encoder import AudioNTT2020Task6
    from src.upstream.delores_s.upstream_expert import Upstream_Expert
    expert = Upstream_Expert(copy.deepcopy(cfg_s), base_encoder=AudioNTT2020Task6)
    fill.fill_state_dict_(expert, seed=9)
    ck = expert.checkpoint()
    ck["hyper_parameters"]["config"] = expert.config                  # as HipTrainer.save_checkpoint writes it
    ck["hyper_parameters"]["base_encoder"] = expert.config["pretrain"]["base_encoder"]["type"]
    path = str(tmp_path / "delores_s.ckpt")
    torch.save(ck, path)
    return path


def test_evaluate_knn_and_store_clusters_commands(tmp_path, cfg_s, capsys):
    import importlib.util
    import types

    import pandas as pd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("evaluate_knn_hip", os.path.join(root, "audio-ssl_amd", "evaluate_knn.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    ckpt = _checkpoint(tmp_path, cfg_s)
    files, _ = _write_wavs(tmp_path, [16000 + 500 * (i % 3) for i in range(12)], salt=300)
    labels = ["dog", "cat", "bird"]
    train = pd.DataFrame({"wav": files[:9], "label": [labels[i % 3] for i in range(9)]})
    test = pd.DataFrame({"wav": files[9:], "label": [labels[i % 3] for i in range(3)]})
    train_csv, test_csv = str(tmp_path / "train.csv"), str(tmp_path / "test.csv")
    train.to_csv(train_csv, index=False)
    test.to_csv(test_csv, index=False)
    dump = str(tmp_path / "dump")
    capsys.readouterr()
    res = ev.main(ev.get_args(["--checkpoint", ckpt, "--upstream", "delores_s", "--train_csv", train_csv, "--test_csv", test_csv,
                               "-k", "5", "--dump_embeddings", dump]))
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out == res
    assert (out["N_train"], out["N_test"], out["d"], out["k"], out["T"]) == (9, 3, 2048, 5, 0.07) and 0.0 <= out["top1"] <= 1.0
    assert np.load(os.path.join(dump, "train_embeddings.npy")).shape == (9, 2048)
    assert np.load(os.path.join(dump, "test_labels.npy")).tolist() == [2, 1, 0]              # sorted ids: bird 0, cat 1, dog 2

    from src.upstream.decar_v2 import store_clusters as sc
    files_csv, out_csv = str(tmp_path / "files.csv"), str(tmp_path / "labelled.csv")
    pd.DataFrame({"files": files}).to_csv(files_csv, index=False)
    np.random.seed(2)
    sc.main(sc.get_args(["--checkpoint", ckpt, "--upstream", "delores_s", "--input", files_csv, "--k", "3", "--out", out_csv,
                         "--pca", "8"]))
    lines = open(out_csv).read().split()
    assert lines[0] == "files,label" and len(lines) == 13
    assert [ln.rsplit(",", 1)[0] for ln in lines[1:]] == files
    assert all(0 <= int(ln.rsplit(",", 1)[1]) < 3 for ln in lines[1:])
    # what `train_upstream.py --upstream unfused` does with that file
    from src.dataset.upstream_dataset import BaseDataset
    ds = BaseDataset(copy.deepcopy(cfg_s), types.SimpleNamespace(upstream="unfused"), out_csv, tfms=None)
    assert len(ds) == 12 and ds.labelled
    wave, label = ds[5]
    assert 0 <= label < 3 and len(wave) == 16000 + 500 * (5 % 3)
