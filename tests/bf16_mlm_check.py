"""Child process of tests/test_gpu_mlm.py::test_bf16_build_mlm: the masked-LM head on the bf16-operand build (OPUS_DTYPE=bf16 ->
libopus_pllm_bf16.so; the library choice is per process).  Prints ONE JSON line of observations; the parent asserts the bounds."""
import json
import os
import sys

os.environ["OPUS_DTYPE"] = "bf16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import opus_pllm_amd as opa  # noqa: E402
from opus_pllm_amd import _cabi, synth  # noqa: E402
from opus_pllm_amd.model import OpusLlamaForCausalLM  # noqa: E402
from opus_pllm_amd.weights import DeviceWeights  # noqa: E402
import mlm_checks as mc  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
cfg = opa.micro()
model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev, mlm_head=True), dev)
out["d64"] = mc.kernel_vs_fp64(model, cfg, synth.mlm_head(cfg, 0))
out["micro"] = mc.micro_vs_fixture(model)
del model
cfg = mc.enc_cfg(1280, 20, 2, 8, 66)
model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev, mlm_head=True), dev)
out["d1280"] = mc.kernel_vs_fp64(model, cfg, synth.mlm_head(cfg, 0))
print("BF16_MLM " + json.dumps(out))
