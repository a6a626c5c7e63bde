"""Child process of tests/test_gpu_attn_decode.py::test_bf16_build_attn_decode: three cases of the decode-attention table on the
bf16-operand build (OPUS_DTYPE=bf16 -> libopus_pllm_bf16.so; the library choice is per process) - a grouped head_dim-16 launch,
the <128, 8> instance on raw slabs with a bias, and a short cache with per-head workgroups.  The peaked family's mass and the
fused family's ambiguous share hold in bf16 as they stand (tests/test_attn_decode_host.py checks both types).  Prints ONE JSON
line of observations; the parent asserts the bounds."""
import json
import os
import sys

os.environ["OPUS_DTYPE"] = "bf16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from opus_pllm_amd import _cabi  # noqa: E402
import attn_decode_checks as ac  # noqa: E402
import attn_decode_ref as R  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype()), "cases": {}}
for name in R.BF16_CASES:
    case = R.CASE_BY_NAME[name]
    r = ac.RawCtx(case.c, dev)
    try:
        out["cases"][name] = ac.run_case(r, case, torch.bfloat16)
    finally:
        r.close()
print("BF16_ATTN_DECODE " + json.dumps(out))
