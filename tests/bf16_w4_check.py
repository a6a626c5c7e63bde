"""Child process of tests/test_gpu_w4.py::test_bf16_build_w4: the MXFP4 decoder weights on the bf16-operand build (OPUS_DTYPE=bf16
-> libopus_pllm_bf16.so; the library choice is per process) - the quantiser against its twin, one cell of every class that has an
MXFP4 form (test_gpu_w4.bf16_cells), and the micro model against its dequantised twin.  Prints ONE JSON line of observations; the
parent asserts."""
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
from opus_pllm_amd.weights import quantize_mxfp4  # noqa: E402
import gemm_cells_checks as K  # noqa: E402
import gemm_cells_ref as R  # noqa: E402
import w4_checks as Q4  # noqa: E402
import w4_ref as W4  # noqa: E402
import test_gpu_w4 as T  # noqa: E402
from gpu_helpers import rel_l2  # noqa: E402

dev = torch.device("cuda:0")
out = {"operand_dtype": int(_cabi.lib().opus_operand_dtype()), "cases": {}}
W = T._weights(48, 192, torch.bfloat16, 1)
q_ref, s_ref, dq_ref = W4.quantize(W)
q4, s4, dq = quantize_mxfp4(W.to(dev))
out["quantiser_is_twin"] = bool(torch.equal(q4.cpu(), W4.tile(q_ref)) and torch.equal(s4.cpu(), W4.tile_scales(s_ref)) and
                                torch.equal(K._bits(dq.cpu()), K._bits(dq_ref)))
ctx = K.make_ctx(opa.llama3_8b(max_batch=64, max_enc_tokens=1026, max_prompt=104, max_new_tokens=16), dev)
for c in T.bf16_cells():
    out["cases"][R.case_id(c)] = Q4.run_exact_case(ctx, dev, c, repeats=2)
_cabi.check(_cabi.lib().opus_check_error(ctx, None))
_cabi.lib().opus_ctx_destroy(ctx)

cfg = opa.micro()
m4, m16 = T._pair(cfg, dev)
ids, mask, seqs = T._ragged(cfg, 3)
emb, mo = T._embed(m16, ids, mask, seqs)
l4, l16 = m4.prefill_logits(emb, mo), m16.prefill_logits(emb, mo)
micro = {"prefill_identical": bool(torch.equal(l4, l16)), "rel_l2": 0.0}
tok = l16.argmax(-1)
for s in range(6):
    a, b = m4.decode_logits(tok), m16.decode_logits(tok)
    micro["rel_l2"] = max(micro["rel_l2"], rel_l2(a, b))
    tok = b.argmax(-1)
micro["w4_gemms"] = m4.stat("w4_gemms")
out["micro"] = micro
print("BF16_W4 " + json.dumps(out))
