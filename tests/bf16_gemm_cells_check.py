"""Child process of tests/test_gpu_gemm_cells.py::test_bf16_build_gemm_cells: gemm_cells_ref.bf16_subset() - one case per
(kernel instantiation, fused norm, epilogue) - on the bf16-operand build (OPUS_DTYPE=bf16 -> libopus_pllm_bf16.so; the library
choice is per process).  The exact family's integers are exact in bf16 as they stand (tests/test_gemm_cells_host.py).  Prints ONE
JSON line of observations; the parent asserts routes, poison checks, bit-exactness and the bounds."""
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
import gemm_cells_checks as K  # noqa: E402
import gemm_cells_ref as R  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype()), "cases": {}}
ctx = K.make_ctx(opa.llama3_8b(max_batch=64, max_enc_tokens=1026, max_prompt=104, max_new_tokens=16), dev)
for c in R.bf16_subset():
    out["cases"][R.case_id(c)] = K.run_case(ctx, dev, c)
_cabi.check(_cabi.lib().opus_check_error(ctx, None))
_cabi.lib().opus_ctx_destroy(ctx)
print("BF16_GEMM_CELLS " + json.dumps(out))
