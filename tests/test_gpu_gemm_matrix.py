"""GPU: every GEMM kernel variant, forced through AUDIOSSL_GEMM_FORCE, against float64 - every layout (the fourth one,
trans_a = 1 / trans_b = 0, included), every epilogue and output mode, split-K down to empty splits, N % 8 != 0, padded leading
dimensions, partial tiles - element by element against a derived bound, with NaN-filled surroundings and bit-checked guard elements
(tests/gemm_cases.py: cases, reference, bound; tests/gemm_matrix_child.py: the program one child process runs per variant).

The other entry points (gemm_multi, gemm_multi_sgd, gemm_multi_barlow, gemm_dropout, moco_logits) run in the same children for the
variants that are legal for them.  Every launch must report the forced family's kernel: each case is legal for its variant, so a
fall-back to the default choice is a failure.

A child that dies - by a signal, an abort, at its time limit, or with its own exit status 70 for an error of the HIP runtime (ELAUNCH
included) - trips a latch: the later tests of this file fail at once without starting another GPU process.  No retries."""
import json
import os
import subprocess
import sys

import pytest

import gemm_cases as G

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEAD_STATUS = (134, 139, 124, 137, 70)        # abort, segmentation fault, time limits, the child's own "HIP runtime error" exit
_dead = []                                     # the latch: why a child died; once set no test of this file starts another GPU process


def _report(variant, lines):
    rows = [json.loads(ln) for ln in lines if ln.startswith("{")]
    fatal = [r for r in rows if "fatal" in r]
    assert not fatal, fatal
    done = [r for r in rows if "done" in r]
    cases = [r for r in rows if "case" in r]
    assert len(done) == 1 and done[0]["done"] == len(cases), "the child did not run to the end"
    want = [c["id"] for c in G.all_cases(variant)]
    assert [r["case"] for r in cases][:len(want)] == want
    k = done[0]["kinds"]
    print(f"{variant or 'default'}: {len(cases)} cases, worst error / bound: fp32 results {k['fp32']:.4f}, bf16 results {k['bf16']:.4f}, "
          f"fixed tolerances {k['tol']:.4f}; {done[0]['seconds']} s")
    bad = [r for r in cases if not r["ok"]]
    assert not bad, f"{len(bad)} of {len(cases)} cases failed:\n" + "\n".join(f"  {r['case']}: {r['why']} (ran {r['kernel']}, ratio {r['ratio']:.3g})" for r in bad)
    assert done[0]["worst"] < 1.0


def _latched():
    if _dead:
        pytest.fail(f"not started: an earlier GEMM matrix child died ({_dead[0]})", pytrace=False)


@pytest.mark.parametrize("variant", G.VARIANTS)
def test_gemm_matrix_forced_variant(variant):
    _latched()
    env = {k: v for k, v in os.environ.items() if k != "AUDIOSSL_GEMM_OFF"}
    env["AUDIOSSL_GEMM_FORCE"] = variant
    try:
        out = subprocess.run([sys.executable, os.path.join(_HERE, "gemm_matrix_child.py"), variant], env=env, capture_output=True, text=True,
                             timeout=240 if variant == "bk32" else 120)
    except subprocess.TimeoutExpired:
        _dead.append(f"{variant}: time limit")
        raise
    if out.returncode < 0 or out.returncode in _DEAD_STATUS:
        _dead.append(f"{variant}: exit status {out.returncode}")
    assert out.returncode == 0, (out.returncode, out.stdout[-1500:], out.stderr[-1500:])
    _report(variant, out.stdout.splitlines())


def test_gemm_matrix_default_choice_and_fp32():
    """In this process (no switch set): the fp32 kernel - a template instance of the register-staged body - through modes (a), (c),
    (d), (e), (f) in every layout, moco_logits under the default choice, and what audiossl_gemm rejects."""
    _latched()
    assert not os.environ.get("AUDIOSSL_GEMM_FORCE") and not os.environ.get("AUDIOSSL_GEMM_OFF"), "the default choice needs both switches unset"
    import gemm_matrix_child as child
    lines = []
    try:
        lines.append(json.dumps(child.run(None, lambda d: lines.append(json.dumps(d)))))
    except child.GpuFault as e:
        _dead.append(f"default: {e}")
        raise
    _report(None, lines)
