"""Child process of tests/test_gpu_guidance.py::test_bf16_build_guidance: the guidance kernel (fp32 arithmetic: the same bounds)
and the micro model's teacher-forced check on the bf16-operand build (OPUS_DTYPE=bf16 -> libopus_pllm_bf16.so; the library choice
is per process).  Prints ONE JSON line of observations; the parent asserts the bounds."""
import json
import os
import sys

os.environ["OPUS_DTYPE"] = "bf16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from opus_pllm_amd import _cabi  # noqa: E402
import guidance_checks as gc  # noqa: E402

dev = torch.device("cuda:0")
model, _ = gc.make_micro(dev)
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype())}
out["kernel"] = gc.kernel(model, dev)
ids, mask, seqs, neg, nmask = gc.micro_inputs(model.cfg)
out["teacher_forced"] = {f"g{g}": gc.teacher_forced(model, ids, mask, seqs, g, gc.MICRO_NEW) for g in (1.5, 3.0)}
print("BF16_GUIDANCE " + json.dumps(out))
