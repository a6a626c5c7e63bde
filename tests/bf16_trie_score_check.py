"""Child process of tests/test_gpu_trie_score.py::test_bf16_build_trie_score: trie scoring on the bf16-operand build
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

import opus_pllm_amd as opa  # noqa: E402
from opus_pllm_amd import _cabi  # noqa: E402
import trie_score_checks as tc  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
out["attn"] = tc.attn_kernel(dev)
out["micro"] = tc.vs_oracle(dev, opa.micro(), P=3, sizes=[12, 5, 20], seed=41, per_row=True)
print("BF16_TRIE_SCORE " + json.dumps(out))
