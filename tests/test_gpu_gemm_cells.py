"""Every cell of the GEMM kernels (tests/gemm_cells_ref.py) on the GPU: each case of the table is launched on a poisoned layout,
the launchers' report (opus_debug_gemm_plan) must be the plan the case is filed under, and the result is held to fp64.

  route        report == the case's plan (kernel class, row tile, ALDS, P, k-parts, how they are combined)
  plain        exact input family: torch.equal with the exact value rounded once to the output type, in all three output modes
  GELU, SiLU   exact family: fp64 of the activation on the exact pre-activation, 2e-3 max |ref| + 1e-5 (the kernel rule)
  fused norm   Gaussian family (the norm cannot be exact): 4e-3 max |ref| + 1e-5, as test_gemm_fused_rmsnorm
  poison       the output is finite, the guard rows behind row M - 1 and A, W, bias are bit-untouched
  repeats      k-parts combined inside the launch (stream combine, pp pair): four launches agree bit for bit
  slabs        opus_debug_gemm_slabs: the slabs, summed, are the exact value bit for bit

Observed GELU / SiLU / fused-norm errors of a run: profiles/gemm_cells_parity.jsonl.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
import gemm_cells_checks as K
import gemm_cells_ref as R
from gpu_helpers import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx(dev):
    """A full-width context without weights: the GEMM workspace (64 MiB), the hand-off words and the QKV scratch of the slab entry."""
    cfg = opa.llama3_8b(max_batch=64, max_enc_tokens=1026, max_prompt=104, max_new_tokens=16)
    c = K.make_ctx(cfg, dev)
    _cabi.check(_cabi.lib().opus_check_error(c, None))
    yield c
    _cabi.check(_cabi.lib().opus_check_error(c, None))       # no hand-off of the module gave up waiting
    _cabi.lib().opus_ctx_destroy(c)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_gemm_cell(ctx, dev, c):
    obs = K.run_case(ctx, dev, c)
    if "exact" not in obs:
        print("gemm_cells", obs["id"], "err", obs["err"], "ref_max", obs["ref_max"], "bound", K.bound(c, obs))
        record("gemm_cells." + obs["id"], {"err": obs["err"], "ref_max": obs["ref_max"], "bound": K.bound(c, obs)})
    bad = K.failures(c, obs)
    assert not bad, (obs["id"], bad)


@pytest.mark.parametrize("c", R.SLAB_CASES, ids=R.case_id)
def test_gemm_slabs_sum_to_the_exact_value(ctx, dev, c):
    obs = K.run_case(ctx, dev, c)
    bad = K.failures(c, obs)
    assert not bad, (obs["id"], bad)


def test_report_is_reset_by_a_refused_gemm(ctx, dev):
    """A GEMM the launcher refuses (gate / up with N % 32 != 0 is caught by the entry; fused norm + fragment-ordered A by the
    launcher) leaves no stale report behind."""
    lib = _cabi.lib()
    c = R.CASES[0]
    K.run_case(ctx, dev, c)
    assert K.report(ctx) == c.plan
    x = torch.zeros(64, 64, dtype=_cabi.operand_dtype(), device=dev)
    o = torch.zeros(64, 64, dtype=_cabi.operand_dtype(), device=dev)
    _cabi.check(lib.opus_debug_knob(ctx, b"debug_a_tiled", 1))
    try:
        rc = lib.opus_debug_gemm(ctx, x.data_ptr(), x.data_ptr(), None, None, o.data_ptr(), 2, 64, 64, 0, 0, None)   # skinny + tiled A
    finally:
        _cabi.check(lib.opus_debug_knob(ctx, b"debug_a_tiled", 0))
    assert rc != 0 and list(K.report(ctx)[1:]) == [-1] * 7


def test_bf16_build_gemm_cells():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_gemm_cells_check.py")], capture_output=True, text=True,
                       env=dict(os.environ, OPUS_DTYPE="bf16"), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_GEMM_CELLS ")][-1]
    o = json.loads(line[len("BF16_GEMM_CELLS "):])
    assert o["operand_dtype"] == 1, o
    cases = {R.case_id(c): c for c in R.bf16_subset()}
    assert sorted(o["cases"]) == sorted(cases)
    record("gemm_cells.bf16", {n: {"err": x["err"], "ref_max": x["ref_max"]} for n, x in o["cases"].items() if "exact" not in x})
    bad = {n: K.failures(cases[n], x, bf16=True) for n, x in o["cases"].items()}
    bad = {n: b for n, b in bad.items() if b}
    assert not bad, bad
