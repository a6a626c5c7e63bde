"""Child process of tests/test_gpu_top_logprobs.py::test_bf16_build_top_logprobs: the top-k kernels and generate(top_logprobs=k)
on the bf16-operand build (OPUS_DTYPE=bf16 -> libopus_pllm_bf16.so; the library choice is per process).  Prints ONE JSON line of
observations; the parent asserts the bounds."""
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
from opus_pllm_amd import _cabi, synth  # noqa: E402
from opus_pllm_amd.model import OpusLlamaForCausalLM  # noqa: E402
from opus_pllm_amd.weights import DeviceWeights  # noqa: E402
import top_logprobs_checks as tlc  # noqa: E402

dev = torch.device("cuda:0")
cfg = opa.micro(max_batch=12)
model = OpusLlamaForCausalLM(cfg, DeviceWeights.from_canonical(cfg, synth.canonical_weights(cfg, 0), dev), dev)
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype()), "kernel": {}, "self": {}}
for V in (96, 128256):
    for f32 in (True, False):
        out["kernel"][f"V{V}.{'fp32' if f32 else 'bf16'}"] = tlc.kernel_cases(model, dev, V, f32)
gold = os.path.join(ROOT, "tests", "golden")
g = dict(np.load(os.path.join(gold, "generate_micro.npz")))
seqs = json.load(open(os.path.join(gold, "generate_micro.seqs.json")))
ids, mask = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])
for name, samp in (("greedy", None), ("sampled", dict(temperature=1.0, top_p=0.9, top_k=50))):
    out["self"][name] = tlc.consistency(tlc.gen(model, ids, mask, seqs, 8, k=5, sampling=samp), 5, True)
print("BF16_TOP_LOGPROBS " + json.dumps(out))
