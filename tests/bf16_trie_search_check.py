"""Child process of tests/test_gpu_trie_search.py::test_bf16_build_trie_search: trie search on the bf16-operand build
(OPUS_DTYPE=bf16 -> libopus_pllm_bf16.so; the library choice is per process).  Prints ONE JSON line of observations; the parent
asserts the bounds."""
import json
import os
import sys

os.environ["OPUS_DTYPE"] = "bf16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import opus_pllm_amd as opa  # noqa: E402
from opus_pllm_amd import _cabi  # noqa: E402
import forward_checks as fc  # noqa: E402
import trie_score_checks as tc  # noqa: E402
import trie_search_checks as ts  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
cfg = opa.micro(max_batch=16)
model = fc.make_model(cfg, dev)
out["kernel"] = ts.expand_kernel(model, cfg.dec_vocab, 2, 8, seed=5)
trie = tc.random_trie(np.random.default_rng(43), 20, hi=4)
out["micro"], _, _ = ts.vs_score_trie(model, cfg, 2, [trie, trie], K=8, top=4, stop=True, seed=44, alone=8 * 1.5e-2)
print("BF16_TRIE_SEARCH " + json.dumps(out))
