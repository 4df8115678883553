"""Runs the GEMM case matrix (gemm_cases.py) in ONE process, i.e. under one value of AUDIOSSL_GEMM_FORCE (the switch is read once
per process):  python gemm_matrix_child.py <variant | default>

One JSON line per case - case id, the kernel the launch reported, the worst |error| / bound, the guard verdict - and a closing
line {"done": cases, "worst": ratio, "kinds": {worst ratio of the fp32 / bf16 / fixed-tolerance results}, "seconds": t}.  Exit status 0 means "ran to the end", whatever the verdicts; an error of the HIP
runtime ends the run at once with status 70 (nothing more is started on a GPU that has reported a fault)."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "audio-ssl_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np
import torch

import gemm_cases as G
from oracle import fill

FATAL_STATUS = 70
_INF = float("inf")


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def _verdict(case, names, ratio, guard, why=""):
    names = list(names)
    expect = case.get("expects") or [case["expect"]] * len(names)
    if names != expect:
        why = (why + " " if why else "") + f"kernel: expected {expect[0] if len(set(expect)) == 1 else expect}"
    if not guard:
        why = (why + " " if why else "") + "guard elements changed"
    if not ratio < 1.0:
        why = (why + " " if why else "") + "over the bound"
    return dict(case=case["id"], kernel=names[-1] if names else "", ratio=ratio, guard=bool(guard), ok=not why, why=why)


def run_gemm(N, E, c):
    fl = dict(G.MODES[c["mode"]])
    p = G.build_problem(c["id"], c["dtype"], c["ta"], c["tb"], c["M"], c["N"], c["K"], **fl)
    C = _dev(p["C0"])
    N.call("gemm", c["dtype"], c["ta"], c["tb"], c["M"], c["N"], c["K"], float(p["alpha"]), _dev(p["A"]), p["lda"], _dev(p["B"]), p["ldb"],
           C, p["ldc"], _dev(p["bias"]), p["relu"], _dev(p["keep"]), p["ldk"], float(p["keep_scale"]), _dev(p["gate"]), p["ldg"],
           fl.get("out_f32", 1), p["atomic"], c["ksplit"], _dev(p["resid"]), p["ldr"])
    name = N.last_kernel()
    torch.cuda.synchronize()
    ratio, nbad, guard = G.check(p, C.cpu())
    return _verdict(c, [name], ratio, guard, f"{nbad} elements" if nbad else "")


def run_multi(N, E, c):
    n = len(c["Ns"])
    ps = [G.build_problem(f"{c['id']}/{i}", 1, c["ta"], c["tb"], c["M"], c["Ns"][i], c["Ks"][i], out_f32=c["out_f32"], alpha=c["alpha"],
                          atomic=c["atomic"]) for i in range(n)]
    As, Bs, Cs = [_dev(p["A"]) for p in ps], [_dev(p["B"]) for p in ps], [_dev(p["C0"]) for p in ps]
    E.gemm_multi(c["ta"], c["tb"], c["M"], c["Ns"], c["Ks"], As, [p["lda"] for p in ps], Bs, [p["ldb"] for p in ps], Cs, [p["ldc"] for p in ps],
                 alpha=c["alpha"], out_f32=c["out_f32"], atomic=c["atomic"], ksplit=c["ksplit"])
    name = N.last_kernel()
    torch.cuda.synchronize()
    res = [G.check(p, C.cpu()) for p, C in zip(ps, Cs)]
    nbad = sum(r[1] for r in res)
    return _verdict(c, [name], max(r[0] for r in res), all(r[2] for r in res), f"{nbad} elements" if nbad else "")


def run_sgd(N, E, c):
    """bit for bit against gemm_multi (fp32 gradient stored) + sgd_momentum, both GEMMs under the same forced variant"""
    M, Ns, K, n = c["M"], c["Ns"], c["K"], len(c["Ns"])
    lr, mu, wd, gs = 0.05, 0.9, 1e-4, 0.5
    u = lambda shape, k, s=1.0: torch.from_numpy(fill.uniform(shape, G.salt(c["id"], k)) * np.float32(s))
    dys = [u((K, M), 10 + i, 0.3).cuda().bfloat16() for i in range(n)]
    xs = [u((K, nn), 20 + i, 0.3).cuda().bfloat16() for i, nn in enumerate(Ns)]
    P0 = [u((M, nn), 30 + i).cuda() for i, nn in enumerate(Ns)]
    M0 = [u((M, nn), 40 + i).cuda() for i, nn in enumerate(Ns)]
    Pa, Ma = [t.clone() for t in P0], [t.clone() for t in M0]
    Ga = [torch.empty(M, nn, device="cuda") for nn in Ns]
    Sa = [torch.empty(M, nn, device="cuda", dtype=torch.bfloat16) for nn in Ns]
    E.gemm_multi(1, 1, M, Ns, [K] * n, dys, [M] * n, xs, Ns, Ga, Ns, out_f32=1, atomic=0)
    names = [N.last_kernel()]
    for p_, g_, m_, s_ in zip(Pa, Ga, Ma, Sa):
        N.call("sgd_momentum", p_, g_, m_, p_.numel(), lr, mu, wd, 0, gs, None, s_, 0)
    Pb, Mb = [t.clone() for t in P0], [t.clone() for t in M0]
    Sb = [torch.empty(M, nn, device="cuda", dtype=torch.bfloat16) for nn in Ns]
    E.gemm_multi_sgd(1, 1, M, Ns, [K] * n, dys, [M] * n, xs, Ns, Pb, Mb, Sb, Ns, (lr, mu, wd, gs, None))
    names.append(N.last_kernel())
    torch.cuda.synchronize()
    same = all(torch.equal(Pb[h], Pa[h]) and torch.equal(Mb[h], Ma[h]) and torch.equal(Sb[h], Sa[h]) for h in range(n))
    moved = all(not torch.equal(Pb[h], P0[h]) for h in range(n))
    c = dict(c, expects=[c["expect_plain"], c["expect"]])
    return _verdict(c, names, 0.0 if same and moved else _INF, True, "" if same else "not bit-identical to gemm_multi + sgd_momentum")


def run_barlow(N, E, c):
    D, Ks, n = c["D"], c["Ks"], len(c["Ks"])
    alpha = 1.0 / 64
    coef, dsc = [0.5, 2.0][:n], [0.01, 0.03][:n]
    td = torch.bfloat16
    A = [G.padded(k, D, fill.uniform((k, D), G.salt(c["id"], 1 + i)), td) for i, k in enumerate(Ks)]
    Bm = [G.padded(k, D, 0.6 * fill.uniform((k, D), G.salt(c["id"], 1 + i)) + 0.8 * fill.uniform((k, D), G.salt(c["id"], 11 + i)), td)
          for i, k in enumerate(Ks)]
    dc0 = torch.full((D + G.GUARD_ROWS, D), G.NAN, dtype=td)
    Ad, Bd, dcs = [_dev(a) for a, _ in A], [_dev(b) for b, _ in Bm], [_dev(dc0) for _ in Ks]
    rep = torch.zeros(n, 32, device="cuda")
    vp, fl, adr = ctypes.c_void_p, ctypes.c_float, ctypes.addressof
    arrs = (E._harr(ctypes.c_int, Ks), E._harr(vp, Ad), E._harr(ctypes.c_long, [ld for _, ld in A]), E._harr(vp, Bd),
            E._harr(ctypes.c_long, [ld for _, ld in Bm]), E._harr(vp, dcs), E._harr(fl, coef), E._harr(fl, dsc), E._harr(vp, [rep[h] for h in range(n)]))
    N.call("gemm_multi_barlow", n, D, adr(arrs[0]), alpha, adr(arrs[1]), adr(arrs[2]), adr(arrs[3]), adr(arrs[4]), adr(arrs[5]),
           adr(arrs[6]), adr(arrs[7]), adr(arrs[8]))
    name = N.last_kernel()
    torch.cuda.synchronize()
    ratio, nbad, guard, why = 0.0, 0, True, ""
    eye = torch.eye(D, dtype=torch.float64)
    for h, k in enumerate(Ks):
        a, b = A[h][0][:k, :D].double(), Bm[h][0][:k, :D].double()
        d = alpha * (a.T @ b) - eye
        ref = dsc[h] * d
        # c = alpha * A^T B as any fp32 result; c - I is one more rounding (the + 8), the identity enters S; then * dscale and the bf16 store
        bound = dsc[h] * 2.0 * (k + 8) * 2.0 ** -24 * (alpha * (a.abs().T @ b.abs()) + eye) + 2.0 ** -8 * ref.abs()
        got = dcs[h].cpu()
        r, nb = G.worst_ratio(got[:D], ref, bound)
        want = coef[h] * float((d * d).sum())
        lrel = abs(float(rep[h].double().sum()) - want) / (1e-4 * want)       # the loss replicas: 1e-4 relative
        if lrel > 1:
            why = f"loss of head {h} off by {lrel * 1e-4:.2e} relative"
        ratio, nbad, guard = max(ratio, r, lrel), nbad + nb, guard and G.guards_intact(got, dc0, D, D)
    return _verdict(c, [name], ratio, guard, why or (f"{nbad} elements" if nbad else ""))


def run_dropout(N, E, c):
    """bit for bit against gemm fed with the mask dropout_mask writes for the same (seed, p, counter)"""
    M, Nn, K = c["M"], c["N"], c["K"]
    A = torch.from_numpy(fill.uniform((M, K), G.salt(c["id"], 1)) * np.float32(0.5)).cuda().bfloat16()
    W = torch.from_numpy(fill.uniform((Nn, K), G.salt(c["id"], 2)) * np.float32(0.2)).cuda().bfloat16()
    bias = torch.from_numpy(fill.uniform((Nn,), G.salt(c["id"], 3))).cuda()
    counter = torch.tensor([41], dtype=torch.int64, device="cuda")
    seed, p = 0x1234ABCD5E, 0.3
    keep = torch.empty(M, Nn, dtype=torch.uint8, device="cuda")
    N.call("dropout_mask", keep, M * Nn, seed, p, counter)
    want = torch.empty(M, Nn, device="cuda", dtype=torch.bfloat16)
    E.gemm(N.BF16, 0, 0, M, Nn, K, A, K, W, K, want, Nn, bias=bias, relu=1, keep=keep, ldk=Nn, keep_scale=1.0 / (1.0 - p))
    names = [N.last_kernel()]
    got = torch.full((M, Nn), G.NAN, device="cuda", dtype=torch.bfloat16)
    N.call("gemm_dropout", 0, 0, M, Nn, K, 1.0, A, K, W, K, got, Nn, bias, 1, seed, p, counter, 1.0 / (1.0 - p))
    names.append(N.last_kernel())
    torch.cuda.synchronize()
    same = torch.equal(got, want) and bool(torch.isfinite(want.float()).all()) and 0.6 < float(keep.float().mean()) < 0.8
    return _verdict(c, names, 0.0 if same else _INF, True, "" if same else "not bit-identical to gemm + dropout_mask")


def run_moco(N, E, c):
    """modes 1 + 2 against float64 log-sum-exp / soft-max with the tolerances of test_moco_fused_softmax_epilogue_vs_materialised_logits:
    lse, loss and dlpos (through moco_lse_merge), P by rel-L2 (that test's bar) and finite everywhere"""
    B, K, dim = c["B"], c["K"], c["dim"]
    nrm = torch.nn.functional.normalize
    qn = nrm(torch.from_numpy(fill.normalish((B, dim), G.salt(c["id"], 1))), dim=1).cuda().bfloat16()
    queue = nrm(torch.from_numpy(fill.normalish((dim, K), G.salt(c["id"], 2))), dim=0).cuda().bfloat16()
    lpos = torch.from_numpy(fill.uniform((B,), G.salt(c["id"], 3), 0.0, 10.0)).cuda()
    T = 0.07
    gscale = 1.0 / (B * T)
    nslot = (K + 63) // 64
    part = torch.full((B, nslot, 2), G.NAN, device="cuda")
    lse, dlpos, loss = torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.zeros(1, device="cuda")
    N.call("moco_logits", 1, qn, queue, B, K, dim, 1.0 / T, part, None, 0.0, None)
    names = [N.last_kernel()]
    N.call("moco_lse_merge", lpos, part, B, nslot, gscale, lse, loss, dlpos)
    P0 = torch.full((B + G.GUARD_ROWS, K), G.NAN, dtype=torch.bfloat16)
    P = P0.cuda()
    N.call("moco_logits", 2, qn, queue, B, K, dim, 1.0 / T, None, lse, gscale, P)
    names.append(N.last_kernel())
    torch.cuda.synchronize()
    logits = torch.cat([lpos.double().cpu()[:, None], qn.double().cpu() @ queue.double().cpu() / T], 1)
    want_lse = torch.logsumexp(logits, 1)
    r_lse = float((lse.double().cpu() - want_lse).abs().max()) / (2e-5 * float(want_lse.abs().max()))
    sm_all = torch.softmax(logits, 1)
    r_loss = abs(float(loss) - float((want_lse - lpos.double().cpu()).mean())) / (1e-5 * float(want_lse.abs().max()))
    want_dl = (sm_all[:, 0] - 1.0) * gscale
    r_dl = float(((dlpos.double().cpu() - want_dl).abs() / (1e-7 + 1e-4 * want_dl.abs())).max())      # rtol 1e-4, atol 1e-7
    sm = sm_all[:, 1:] * gscale
    Pc = P.cpu()
    finite = bool(torch.isfinite(Pc[:B].float()).all()) and bool(torch.isfinite(part).all())
    r_p = float((Pc[:B].double() - sm).norm() / sm.norm()) / 4e-3
    ratio = max(r_lse, r_p, r_loss, r_dl) if finite else _INF
    return _verdict(c, names, ratio, G.guards_intact(Pc, P0, B, K), "" if finite else "non-finite partials or probabilities")


def rejected(N):
    """what the entry point refuses, one assertion each -> verdict lines"""
    a = torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16)
    f = torch.zeros(64, 64, device="cuda")
    ptr = lambda t: t.data_ptr()
    lib = N.lib()
    rcs = {
        # ReLU with split-K
        "reject-relu-splitk": (lib.audiossl_gemm(1, 0, 0, 64, 64, 64, 1.0, ptr(a), 64, ptr(a), 64, ptr(f), 64, None, 1, None, 0, 1.0, None, 0, 1, 1, 2, None, 0, None), -1),
        # residual with an accumulating output
        "reject-resid-atomic": (lib.audiossl_gemm(1, 0, 0, 64, 64, 64, 1.0, ptr(a), 64, ptr(a), 64, ptr(f), 64, None, 0, None, 0, 1.0, None, 0, 1, 2, 1, ptr(f), 64, None), -1),
        # N % 8 != 0 with a transposed B ([K][N]: N is the vector dimension)
        "reject-n-mod-8-transb": (lib.audiossl_gemm(1, 0, 1, 64, 60, 64, 1.0, ptr(a), 64, ptr(a), 64, ptr(f), 64, None, 0, None, 0, 1.0, None, 0, 1, 0, 1, None, 0, None), -1),
    }
    return [dict(case=k, kernel="", ratio=0.0, guard=True, ok=rc == want, why="" if rc == want else f"returned {rc}, expected {want}")
            for k, (rc, want) in rcs.items()]


RUNNERS = {"gemm": run_gemm, "gemm_multi": run_multi, "gemm_multi_sgd": run_sgd, "gemm_multi_barlow": run_barlow, "gemm_dropout": run_dropout,
           "moco_logits": run_moco}


class GpuFault(Exception):
    pass


def run(variant, emit):
    """variant: a name of gemm_cases.VARIANTS, or None for the default choice.  emit(dict) per case; -> closing dict."""
    from src import _native as N
    from src import engine as E
    forced = os.environ.get("AUDIOSSL_GEMM_FORCE")
    if forced != variant or os.environ.get("AUDIOSSL_GEMM_OFF"):
        raise RuntimeError(f"AUDIOSSL_GEMM_FORCE={forced!r} in the environment, the cases are those of {variant!r}")
    N.lib()
    t0 = time.time()
    # worst ratio by kind of result: fp32 (accumulation error only), bf16 (the store's own 2^-8 rounding is part of the bound, so the ratio
    # comes close to 1 by construction), tol (moco_logits: against that test's fixed tolerances; the bit-for-bit cases report 0)
    worst, n, kinds = 0.0, 0, {"fp32": 0.0, "bf16": 0.0, "tol": 0.0}
    for c in G.all_cases(variant):
        try:
            v = RUNNERS[c["entry"]](N, E, c)
        except RuntimeError as e:
            # only a refused argument (EINVAL / EALIGN) is a verdict; ELAUNCH is how a sticky HIP error surfaces at the next launch
            if "AUDIOSSL_EINVAL" not in str(e) and "AUDIOSSL_EALIGN" not in str(e):
                raise GpuFault(f"{c['id']}: {e}")
            v = dict(case=c["id"], kernel="", ratio=_INF, guard=True, ok=False, why=str(e))
        emit(v)
        worst, n = max(worst, v["ratio"]), n + 1
        kind = G.result_kind(c)
        kinds[kind] = max(kinds[kind], v["ratio"])
    if variant is None:
        for v in rejected(N):
            emit(v)
            n += 1
    return dict(done=n, worst=worst, kinds=kinds, seconds=round(time.time() - t0, 2))


def main():
    variant = None if sys.argv[1] == "default" else sys.argv[1]
    emit = lambda d: print(json.dumps(d), flush=True)
    try:
        emit(run(variant, emit))
    except GpuFault as e:
        emit(dict(fatal=str(e)))
        sys.stdout.flush()
        os._exit(FATAL_STATUS)


if __name__ == "__main__":
    main()
