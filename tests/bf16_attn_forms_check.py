"""Child process of tests/test_gpu_attn_forms.py::test_bf16_build_attn_forms: one token-packed q_trim case and one causal case of
the form table, both with two query tiles per wave and both input families, on the bf16-operand build (OPUS_DTYPE=bf16 ->
libopus_pllm_bf16.so; the library choice is per process).  The peaked family's 0.99 mass condition holds in bf16 as it stands
(tests/test_attn_forms_host.py checks it for both types).  Prints ONE JSON line of observations; the parent asserts the bounds."""
import json
import os
import sys

os.environ["OPUS_DTYPE"] = "bf16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import opus_pllm_amd as opa  # noqa: E402
from opus_pllm_amd import _cabi  # noqa: E402
import attn_forms_checks as ac  # noqa: E402
import attn_forms_ref as R  # noqa: E402
import forward_checks as fc  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype()), "cases": {}}
model = fc.make_model(opa.micro(), dev)
for name in ("packed_hd64_qt2_trim1", "dec_hd64_qt2"):
    out["cases"][name] = ac.run_case(dev, model._ctx, R.CASE_BY_NAME[name], torch.bfloat16)
print("BF16_ATTN_FORMS " + json.dumps(out))
