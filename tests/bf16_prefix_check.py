"""Child process of tests/test_gpu_prefix.py::test_bf16_build_prefix: shared-prefix scoring on the bf16-operand build
(OPUS_DTYPE=bf16 -> libopus_pllm_bf16.so; the library choice is per process).  Prints ONE JSON line of observations; the parent
asserts the bounds."""
import json
import os
import sys

os.environ["OPUS_DTYPE"] = "bf16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from opus_pllm_amd import _cabi  # noqa: E402
import prefix_checks as pc  # noqa: E402
from test_gpu_forward import _llama8b_2layer  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
out["attn"] = pc.attn_kernel(dev)
out["llama8b"] = pc.vs_forward(dev, _llama8b_2layer(), P=6, K=3, seed=11)
print("BF16_PREFIX " + json.dumps(out))
