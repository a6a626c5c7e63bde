"""attn_decode_kernel at kernel level in all of its 16 instances (head_dim 16 / 32 / 64 / 128 x 1 / 2 / 4 / 8 query heads per
workgroup) and both input forms: finished projections, and the raw split-K slabs + sums of squares + bias that the decode step
hands it at 4 < B <= 64, with the output row-major and fragment-ordered.  Launched through opus_debug_attn_decode_form, compared
with the fp64 reference of tests/attn_decode_ref.py on caches of 1 .. 159 slots (idle waves, the new key first / last / alone in
its tile, kstart inside the new key's tile, the context's last slot); the case table, the cells of the kernel's tiling it reaches
and the premises of the inputs are checked on the CPU by tests/test_attn_decode_host.py.

Bounds: max |O - ref| <= 4e-3 (tests/test_gpu_longctx.py, test_gpu_parity.py::test_attention_kernel); the appended key within
2e-3 max |ref|; the appended value bit-exact - in the fused form equal to the rounding of the fp64 projection wherever fp32 can
decide it, elsewhere a rounding of a value inside the fp32 evaluation's error (one step off at most wherever that error is
below half a step).  Everything else is exact: the GP the launcher reports, a second launch, the
fragment-ordered output against the row-major one, a row alone against the row in its batch, the inputs afterwards, and the
cache: exactly slot L of every (row, kv head) is written, every other slot keeps its bits, NaN patterns included."""
import json
import os
import subprocess
import sys

import pytest
import torch

import attn_decode_checks as ac
import attn_decode_ref as R
from gpu_helpers import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ATTN_ABS = 4e-3            # the project's attention rule
ATTN_ABS_BF16 = 2.4e-2     # tests/test_gpu_bf16.py: the bf16 build's attention bound


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", [c.name for c in R.CONTEXTS])
def test_attn_decode_context(dev, name):
    """Every case of one (head_dim, group) context: the per-head instance at batch 7 and the grouped one at batch 64, ten cache
    lengths, the random and the peaked family, and on three contexts the fused input in all eight slab counts."""
    r = ac.RawCtx(R.CTX_BY_NAME[name], dev)
    bad = {}
    try:
        for case in R.cases_of(name):
            obs = ac.run_case(r, case)
            record("attn_decode." + case.name, ac.summary(obs))
            print(case.name, json.dumps(obs))
            b = ac.failures(case, obs, ATTN_ABS)
            if b:
                bad[case.name] = (b, obs)
    finally:
        r.close()
        torch.cuda.empty_cache()
    assert not bad, bad


def test_entry_refusals_launch_nothing(dev):
    """Null pointers, both or neither input form, B / T0 / step outside the context, ks outside 1 .. 8, no sums-of-squares
    blocks and slabs without sums of squares: each comes back with its code, reports GP 0 and leaves a sentinel-filled O as it
    was."""
    r = ac.RawCtx(R.CTX_BY_NAME["hd16_g3"], dev)
    try:
        res = ac.refusals(r)
    finally:
        r.close()
    print(res)
    assert len(res) == 15
    assert all(rc == want and gp == 0 and kept for rc, want, gp, kept in res.values()), res


def test_bf16_build_attn_decode():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_attn_decode_check.py")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("BF16_ATTN_DECODE ")][-1]
    o = json.loads(line[len("BF16_ATTN_DECODE "):])
    record("attn_decode.bf16", {n: ac.summary(x) for n, x in o["cases"].items()})
    print(o)
    assert o["operand_dtype"] == 1, o
    assert sorted(o["cases"]) == sorted(R.BF16_CASES), o
    for n, obs in o["cases"].items():
        bad = ac.failures(R.CASE_BY_NAME[n], obs, ATTN_ABS_BF16, ac.K_REL_BF16)
        assert not bad, (n, bad, obs)
