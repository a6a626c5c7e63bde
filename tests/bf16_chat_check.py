"""Child process of tests/test_gpu_chat.py::test_bf16_build_chat: the ragged export and a conversation's later turns on the
bf16-operand build (OPUS_DTYPE=bf16 -> libopus_pllm_bf16.so; the library choice is per process).  Prints ONE JSON line of
observations; the parent asserts the bounds."""
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
import chat_checks as cc  # noqa: E402
import forward_checks as fc  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
model = fc.make_model(opa.micro(), dev)
out["export"] = cc.export_checks(model, seed=11)
out["turns"] = cc.turns_vs_concat(model, seed=21)
print("BF16_CHAT " + json.dumps(out))
