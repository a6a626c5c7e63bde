"""Child process of tests/test_gpu_w8.py::test_bf16_build_w8: the FP8 decoder weights on the bf16-operand build (OPUS_DTYPE=bf16
-> libopus_pllm_bf16.so; the library choice is per process) - the quantiser against its twin, the cells of
gemm_cells_ref.bf16_subset() that have an FP8 form, and the micro model against its dequantised twin.  Prints ONE JSON line of
observations; the parent asserts."""
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
from opus_pllm_amd.weights import quantize_fp8  # noqa: E402
import gemm_cells_checks as K  # noqa: E402
import gemm_cells_ref as R  # noqa: E402
import w8_checks as Q  # noqa: E402
import w8_ref as W8  # noqa: E402
import test_gpu_w8 as T  # noqa: E402
from gpu_helpers import rel_l2  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype()), "cases": {}}
W = T._weights(48, 192, torch.bfloat16, 1)
q_ref, e_ref, dq_ref = W8.quantize(W)
q8, e8, dq = quantize_fp8(W.to(dev))
out["quantiser_is_twin"] = bool(torch.equal(q8.cpu(), W8.tile(q_ref)) and torch.equal(e8.cpu(), e_ref) and
                                torch.equal(K._bits(dq.cpu()), K._bits(dq_ref)))
ctx = K.make_ctx(opa.llama3_8b(max_batch=64, max_enc_tokens=1026, max_prompt=104, max_new_tokens=16), dev)
for c in R.bf16_subset():
    if c.plan.klass in Q.W8_CLASSES:
        out["cases"][R.case_id(c)] = Q.run_exact_case(ctx, dev, c, repeats=2)
_cabi.check(_cabi.lib().opus_check_error(ctx, None))
_cabi.lib().opus_ctx_destroy(ctx)

cfg = opa.micro()
m8, m16 = T._pair(cfg, dev)
ids, mask, seqs = T._ragged(cfg, 3)
emb, mo = T._embed(m16, ids, mask, seqs)
l8, l16 = m8.prefill_logits(emb, mo), m16.prefill_logits(emb, mo)
micro = {"prefill_identical": bool(torch.equal(l8, l16)), "rel_l2": 0.0}
tok = l16.argmax(-1)
for s in range(6):
    a, b = m8.decode_logits(tok), m16.decode_logits(tok)
    micro["rel_l2"] = max(micro["rel_l2"], rel_l2(a, b))
    tok = b.argmax(-1)
micro["w8_gemms"] = m8.stat("w8_gemms")
out["micro"] = micro
print("BF16_W8 " + json.dumps(out))
