"""Child process of tests/test_gpu_nsamples.py::test_bf16_build_nsamples: the fanned-out prefill and generate(num_return_sequences=N)
on the bf16-operand build (OPUS_DTYPE=bf16 -> libopus_pllm_bf16.so; the library choice is per process).  Prints ONE JSON line of
observations; the parent asserts the bounds."""
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
import nsamples_checks as nsc  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
model, B, N, lens = nsc.micro_model("micro_3x3", dev)
out["micro_3x3"] = {"replicas": nsc.prefill_and_replicas(model, dev, B, N, lens),
                    "reference_mode": nsc.sampled(model, dev, B, N, lens, nsc.REFERENCE_MODE),
                    "open_mode": nsc.sampled(model, dev, B, N, lens, nsc.OPEN_MODE)}
del model
big = gsc.make_model(gsc.llama8b_shape(64, 2, 8), dev)
B, N, lens = nsc.BIG_CASES["llama8b_12x5"]
out["llama8b_12x5"] = {"replicas": nsc.prefill_and_replicas(big, dev, B, N, lens),
                       "reference_mode": nsc.sampled(big, dev, B, N, lens, nsc.REFERENCE_MODE, max_new=2),
                       "open_mode": nsc.sampled(big, dev, B, N, lens, nsc.OPEN_MODE, max_new=2)}
print("BF16_NSAMPLES " + json.dumps(out))
