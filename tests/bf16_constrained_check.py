"""Child process of tests/test_gpu_constrained.py::test_bf16_build_constrained: the constraint kernel and greedy generate() under
a 50 000-member trie on the bf16-operand build (OPUS_DTYPE=bf16 -> libopus_pllm_bf16.so; the library choice is per process).
Prints ONE JSON line of observations; the parent asserts the bounds."""
import json
import os
import sys

os.environ["OPUS_DTYPE"] = "bf16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from opus_pllm_amd import _cabi  # noqa: E402
import constrained_checks as cc  # noqa: E402
import gen_scores_checks as gsc  # noqa: E402

dev = torch.device("cuda:0")
model = gsc.make_model(gsc.llama8b_shape(B=64, layers=2, max_new=16), dev)
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
out["kernel"] = cc.kernel(model, dev)
out["big"] = cc.big(model, dev, B=64, max_new=16, sampling=False)
print("BF16_CONSTRAINED " + json.dumps(out))
