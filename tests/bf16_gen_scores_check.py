"""Child process of tests/test_gpu_gen_scores.py::test_bf16_build_gen_scores: generate()'s output kernels on the bf16-operand
build (OPUS_DTYPE=bf16 -> libopus_pllm_bf16.so; the library choice is per process).  Prints ONE JSON line of observations; the
parent asserts the bounds."""
import json
import os
import sys

os.environ["OPUS_DTYPE"] = "bf16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from opus_pllm_amd import _cabi  # noqa: E402
import gen_scores_checks as gsc  # noqa: E402

dev = torch.device("cuda:0")
model = gsc.make_model(gsc.llama8b_shape(B=64, layers=2, max_new=8), dev)
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
out["kernel"] = gsc.argmax_lse_kernel(model, dev)
out["self"] = gsc.self_consistency(model, dev, B=64, max_new=8)
print("BF16_GEN_SCORES " + json.dumps(out))
