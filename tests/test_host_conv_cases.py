"""CPU: the exact 3x3 convolution cases (tests/conv_cases.py) that tests/test_gpu_conv_matrix.py holds the kernels to - the shape list
reaches the edges it claims, the premise (float64 = fp32, bit for bit) holds, the bf16 rounding is really exercised, and the bit
comparison sees a truncating conversion, a negative zero and a single changed element."""
import torch

import conv_cases as C

SMALL = [s for s in C.SHAPES if C.tiles(s) <= 4]


def test_conv_cases_shapes_reach_the_edges():
    assert len(set(C.SHAPES)) == len(C.SHAPES) == 25 and set(C.ISOLATION_SHAPES) <= set(C.SHAPES)
    for fi in (32, 16):
        shapes = [s for s in C.SHAPES if s[2] == fi]
        tt = 256 // fi
        assert {256, 257, 513} <= {C.tiles(s) for s in shapes}
        assert any(ti == 1 and n > 1 for n, ti, _ in shapes) and any(ti == 2 and n > 1 for n, ti, _ in shapes)      # all rows are borders
        assert any(n > 1 and ti % tt == 0 and C.tiles((n, ti, fi)) < 256 for n, ti, _ in shapes)                    # border on a tile border
        assert any(n > 1 and ti % tt for n, ti, _ in shapes)                                                         # border inside a tile
        assert any(C.tiles(s) == 257 and (s[0] * s[1]) % tt == 1 and (s[0] * s[1]) % 2 == 1 for s in shapes)         # one-row last tile
        assert any(C.tiles(s) == 257 and (s[0] * s[1]) % tt == 0 for s in shapes)
        assert max(n * ti * fi * 64 * 2 for n, ti, _ in shapes) <= 17 << 20                                          # bf16 bytes of the largest x


def test_conv_cases_premise_holds_on_the_small_shapes():
    """fwd_ref / wgrad_ref assert it themselves (every float64 result an fp32 number, the CPU's fp32 convolution equal to it, no negative
    zero); here they run for every shape of at most four tiles, and the inputs are what the docstring says"""
    for s in SMALL:
        c = C.inputs(s)
        assert int(c["x"].float().abs().max()) <= 2 and int(c["dy"].float().abs().max()) <= 2
        assert float((c["w"] * 64).abs().max()) <= 16 and torch.equal((c["w"] * 64).round(), c["w"] * 64)
        assert float((c["bias"] * 64).abs().max()) <= 32 and torch.equal(c["dw0"].round(), c["dw0"])
        r = C.fwd_ref(s, fp32_too=True)
        assert r["y"].shape == c["x"].shape and r["dx"].shape == c["x"].shape
        assert torch.equal(r["y"] - r["y0"], c["bias"].expand_as(r["y"]))
        assert C.wgrad_ref(s, fp32_too=True).shape == (64, 64, 3, 3)


def test_conv_cases_bits_see_a_truncating_conversion():
    y = C.fwd_ref((3, 8, 32), fp32_too=True)["y"]
    rne = y.bfloat16()
    assert float((rne.float() != y).float().mean()) > 0.15                        # the rounding is exercised ...
    trunc = (C.bits(y) >> 16).to(torch.int16).view(torch.bfloat16)
    k = C.mismatches(trunc, rne)
    assert 0 < k < y.numel() // 4                                                 # ... and a truncation changes some elements, not most
    rel = float((trunc.double() - y.double()).norm() / y.double().norm())
    assert rel < 4e-3                                                             # which a relative L2 bound of 4e-3 does not see
    assert C.mismatches(rne, rne.clone()) == 0
    one = rne.clone()
    one.view(-1)[12345] += 1
    assert C.mismatches(one, rne) == 1
    assert C.mismatches(torch.tensor([-0.0, float("nan")]), torch.tensor([0.0, float("nan")])) == 1
