"""Child process of tests/test_gpu_logits_proc.py::test_bf16_build_logits_proc: the logits-processor kernel and greedy generate()
with processors on the bf16-operand build (OPUS_DTYPE=bf16 -> libopus_pllm_bf16.so; the library choice is per process).  Prints
ONE JSON line of observations; the parent asserts the bounds."""
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
import logits_proc_checks as lpc  # noqa: E402

dev = torch.device("cuda:0")
model = gsc.make_model(gsc.llama8b_shape(B=64, layers=2, max_new=16), dev)
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
out["kernel"] = lpc.kernel(model, dev)
out["big"] = lpc.big(model, dev, B=64, max_new=16, sampling=False)
print("BF16_LOGITS_PROC " + json.dumps(out))
