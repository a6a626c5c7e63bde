"""attn_prefill_kernel at kernel level in every form the product launches: token-packed (the encoder's default), token-packed
with q_trim (its last layer), padded with kend (the padded encoder) and causal with kstart and GQA (the decoder prefill), each
with one and with two 16-query tiles per wave, on Q / K / V that are column ranges of one fused projection buffer.  Launched
through opus_debug_attn_prefill, compared with the fp64 reference of tests/attn_forms_ref.py on two input families; the case
table, the cells of the kernel's tiling it reaches and the premises of the inputs are checked on the CPU by
tests/test_attn_forms_host.py.

Bound: max |O - ref| <= 4e-3 over every computed query with a visible key, the rule of test_gpu_parity.py::test_attention_kernel
(fp16 operands, fp32 accumulation, fp16 probabilities and output; unit-normal V).  Everything else is exact: rows without a
visible key are zero, rows the launch must not write keep the bit pattern O was filled with, a protein alone / a second launch /
q_trim off give the same bits."""
import json
import os
import subprocess
import sys

import pytest
import torch

import opus_pllm_amd as opa
import attn_forms_checks as ac
import attn_forms_ref as R
import forward_checks as fc
from gpu_helpers import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ATTN_ABS = 4e-3            # tests/test_gpu_parity.py::test_attention_kernel
ATTN_ABS_BF16 = 2.4e-2     # tests/test_gpu_bf16.py: the bf16 build's attention bound


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx(dev):
    model = fc.make_model(opa.micro(), dev)          # (any context: the entry uses its device and timing records only)
    yield model._ctx
    del model


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_attn_prefill_form(dev, ctx, case):
    """Both input families of one table case: parity with fp64 within 4e-3, the expected QT, zeros where no key is visible, the
    sentinel in trimmed rows (every row of a 2-token protein) and guard rows, Q / K / V untouched, a second launch bit-identical;
    token-packed cases also every protein alone bit-identical to its rows in the batch, q_trim cases bit-identical to q_trim = 0
    on the rows both compute."""
    obs = ac.run_case(dev, ctx, case)
    record("attn_forms." + case.name, {f: {k: o[k] for k in ("err", "qt_used", "rows_checked", "rows_dark") + (("mass",) if "mass" in o else ())}
                                       for f, o in obs.items()})
    print(case.name, json.dumps(obs))
    bad = ac.failures(case, obs, ATTN_ABS)
    assert not bad, (bad, obs)
    if case.form == "packed":
        assert all(o["alone_runs"] == case.B - (1 if case.trim else 0) for o in obs.values()), obs
        assert all(("trim_equals_full_bitwise" in o) == bool(case.trim) for o in obs.values()), obs
    if case.form == "decoder":
        assert all(o["rows_dark"] > 0 for o in obs.values()) or max(case.kstart) == 0, obs


def test_launcher_refusals_launch_nothing(dev, ctx):
    """A stride the 16-byte loads / 8-byte stores cannot take, byte offsets that reach 2^31, a head_dim without an instance,
    causal with cu and q_trim without cu: each comes back as an error, reports no QT and leaves a sentinel-filled O as it was."""
    res = ac.refusals(dev, ctx)
    print(res)
    want = {"q_stride_not_multiple_of_8": -3, "o_stride_not_multiple_of_4": -3, "k_offsets_reach_2^31": -3, "v_offsets_reach_2^31": -3,
            "head_dim_48": -3, "causal_with_cu": -5, "q_trim_without_cu": -2}
    assert {k: v[0] for k, v in res.items()} == want, res
    assert all(qt == 0 and kept for _, qt, kept in res.values()), res


def test_bf16_build_attn_forms():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_attn_forms_check.py")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_ATTN_FORMS ")][-1]
    o = json.loads(line[len("BF16_ATTN_FORMS "):])
    record("attn_forms.bf16", {n: {f: x["err"] for f, x in c.items()} for n, c in o["cases"].items()})
    print(o)
    assert o["operand_dtype"] == 1, o
    assert sorted(o["cases"]) == ["dec_hd64_qt2", "packed_hd64_qt2_trim1"], o
    for name, obs in o["cases"].items():
        bad = ac.failures(R.CASE_BY_NAME[name], obs, ATTN_ABS_BF16)
        assert not bad, (name, bad, obs)
