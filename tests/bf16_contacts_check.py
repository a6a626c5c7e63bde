"""Child process of tests/test_gpu_contacts.py::test_bf16_build_contacts: contact maps on the bf16-operand build
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
from opus_pllm_amd import _cabi, synth  # noqa: E402
from opus_pllm_amd.model import OpusLlamaForCausalLM  # noqa: E402
from opus_pllm_amd.weights import DeviceWeights  # noqa: E402
import contact_checks as cc  # noqa: E402

dev = torch.device("cuda:0")
cfg = opa.micro()
model = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev, contact_head=True), dev)
W = {k: torch.from_numpy(v) for k, v in synth.canonical_weights(cfg, 0).items()}     # (bf16-rounded in this process)
seqs = [synth.synth_protein(n, i) for i, n in enumerate((40, 17, 1, 64))]
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
out["kernel"] = cc.kernel_vs_fp64(dev, model._ctx, 16)
out["micro"] = cc.model_vs_oracle(model, cfg, seqs, W, synth.contact_head(cfg, 0))
enc = model.get_protein_encoder()
_, m1 = enc.get_amino_acid_embeddings(seqs, return_contacts=True)
_, m2 = enc.get_amino_acid_embeddings(seqs, return_contacts=True)
out["bitwise"] = all(torch.equal(a, b) for a, b in zip(m1, m2))
print("BF16_CONTACTS " + json.dumps(out))
