"""CPU: the GEMM case matrix itself (tests/gemm_cases.py) - coverage of the generator, and that the float64 reference and the
per-element bound accept an honest fp32 result and reject the defects the matrix exists for."""
import pytest
import torch

import gemm_cases as G


def test_every_variant_covers_every_layout_and_mode():
    for v in G.VARIANTS:
        cases = G.single_cases(v)
        assert {(c["ta"], c["tb"]) for c in cases} == set(G.LAYOUTS), v
        if v == "bk32":
            assert len(cases) <= 5
            continue
        pairs = {(c["ta"], c["tb"], c["mode"]) for c in cases}
        assert pairs >= {(ta, tb, m) for ta, tb in G.LAYOUTS for m in "abcdef"}, v
        if v not in ("reg64x128", "reg128_k64", "reg128_k128"):      # the residual through the one-column epilogue too (the reg shapes have N = 105)
            assert pairs >= {(ta, tb, "do") for ta, tb in G.LAYOUTS}, v
        for ta, tb in G.LAYOUTS:
            assert {c["ksplit"] for c in cases if c["mode"] == "f" and (c["ta"], c["tb"]) == (ta, tb)} >= {2, 3, 8}, v
            assert any(c["N"] % 8 == 0 and c["mode"] == "b" for c in cases if (c["ta"], c["tb"]) == (ta, tb)), v     # the vector epilogue
            if not tb:
                assert any(c["N"] % 8 for c in cases if (c["ta"], c["tb"]) == (ta, tb)), v
    assert {c["mode"] for c in G.single_cases(None)} == set("acdef")
    for v in G.MULTI_VARIANTS:
        assert {(c["ta"], c["tb"]) for c in G.multi_cases(v)} == set(G.LAYOUTS)
        assert G.sgd_case(v) and G.dropout_cases(v)
    assert all(G.barlow_cases(v) for v in G.MULTI_VARIANTS if v != "reg128_k128") and G.moco_cases("p8") and G.moco_cases("sp8")


def _fp32_result(p, ksplit_bias=1, drop_k=0, gate_ge=False):
    """the epilogue in fp32 on the CPU, with optional defects"""
    a, b = p["opA"].float(), p["opB"].float()
    if drop_k:
        a, b = a[:, :-drop_k], b[:-drop_k]
    x = torch.tensor(p["alpha"], dtype=torch.float32) * (a @ b)
    M, N = p["M"], p["N"]
    if p["bias"] is not None:
        x = x + ksplit_bias * p["bias"]
    if p["relu"]:
        x = x.clamp_min(0)
    if p["keep"] is not None:
        x = torch.where(p["keep"][:M, :N] != 0, x * torch.tensor(p["keep_scale"], dtype=torch.float32), torch.zeros_like(x))
    if p["gate"] is not None:
        g = p["gate"][:M, :N].float()
        x = torch.where((g >= 0) if gate_ge else (g > 0), x, torch.zeros_like(x))
    if p["resid"] is not None:
        x = x + p["resid"][:M, :N]
    C = p["C0"].clone()
    C[:M, :N] = (C[:M, :N].float() + x if p["atomic"] else x).to(C.dtype)
    return C


@pytest.mark.parametrize("mode,dtype", [(m, d) for d in (0, 1) for m in ("acdef" if d == 0 else "abcdef")])
def test_reference_and_bound(mode, dtype):
    ta, tb = (1, 0) if mode in "ace" else (0, 1)
    M, N = G.fit(ta, tb, 72, 105)
    p = G.build_problem(f"host-{mode}-{dtype}", dtype, ta, tb, M, N, 448, **G.MODES[mode])
    ratio, nbad, guard = G.check(p, _fp32_result(p))
    assert ratio < 1.0 and nbad == 0 and guard, ratio
    assert G.check(p, _fp32_result(p, drop_k=64))[1] > 0                       # a dropped K-tile
    if p["bias"] is not None:
        assert G.check(p, _fp32_result(p, ksplit_bias=2))[1] > 0               # the bias added twice
    if p["gate"] is not None:
        assert G.check(p, _fp32_result(p, gate_ge=True))[1] > 0                # +0.0 / -0.0 must zero the output
    C = _fp32_result(p)
    C[M, 0] = 1.0                                                              # a guard row written
    assert not G.check(p, C)[2]
    C = _fp32_result(p)
    C[0, N] = C[0, N - 1]                                                      # a guard column written
    assert not G.check(p, C)[2]
    C = _fp32_result(p)
    C[3, 5] = float("nan")
    assert G.check(p, C)[0] == float("inf")
