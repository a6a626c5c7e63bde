"""Child process of tests/test_gpu_lookup.py::test_bf16_build_lookup: prompt-lookup decoding on the bf16-operand build
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
import lookup_checks as LC  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
micro = LC.make_model(opa.micro(max_batch=64, max_prompt=96, max_new_tokens=24), dev)
bad = 0
for L in (2, 257):
    bad += len(LC.draft_mismatches(micro._lib, micro._ctx, dev, LC.draft_histories(3, L, 5, L), 7, 2))
bad += len(LC.draft_mismatches(micro._lib, micro._ctx, dev, LC.sentinel_histories(), 7, 2))
out["draft_mismatches"] = bad
out["micro_rel_l2"] = max(LC.verify_vs_prefill(micro, R, Tp, pads, n, seed=Tp)["rel_l2"]
                          for R, Tp, pads, n in ((3, 31, [0, 7, 3], 8), (3, 62, [33, 0, 7], 16), (1, 64, [7], 2)))
out["stale"] = LC.stale_slots(micro)
out["kv"] = LC.verify_kv(micro, 3, 62, [0, 7, 33], 8, seed=62)
small = LC.make_model(opa.micro(max_batch=24), dev)
g = np.load(os.path.join(ROOT, "tests", "golden", "generate_micro.npz"))     # (ids decided by margins of 0.10 or more)
seqs = json.load(open(os.path.join(ROOT, "tests", "golden", "generate_micro.seqs.json")))
ids, mask = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])
plain, got, stats = LC.e2e(small, ids, mask, seqs, 12, k=7)
plain2, got2, stats2 = LC.e2e(small, ids, mask, seqs, 12, k=7, lookup_ids=plain)
out["e2e_equal"] = bool(torch.equal(plain, got) and torch.equal(plain2, got2))
out["e2e_accepted"] = stats2.accepted
del micro, small
wide = LC.make_model(LC.wide_cfg(64), dev)
out["wide_rel_l2"] = max(LC.verify_vs_prefill(wide, R, Tp, pads, n, seed=Tp)["rel_l2"]
                         for R, Tp, pads, n in ((3, 31, [0, 7, 3], 8), (4, 64, [0, 7, 33, 1], 16)))
print("BF16_LOOKUP " + json.dumps(out))
