"""CPU checks of tests/gemm_cells_ref.py: the cell list is filled, no case's restated route contradicts the cell it is filed
under, the exact input family is exact, and the restatement's reading of the older parity tuples."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cells_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_cell_has_a_case():
    assert len(set(R.CELLS)) == len(R.CELLS) and not set(R.CELLS) & set(R.SLAB_CELLS) and not set(R.CELLS) & set(R.EXTRA_CELLS)
    filled = {R.cell_of(c) for c in R.CASES}
    assert [c for c in R.CELLS + R.EXTRA_CELLS if c not in filled] == []
    assert sorted(filled - set(R.CELLS)) == sorted(R.EXTRA_CELLS)          # and no case sits in a cell nobody listed
    assert {R.cell_of(c) for c in R.SLAB_CASES} == set(R.SLAB_CELLS)
    ids = [R.case_id(c) for c in R.CASES + R.SLAB_CASES]
    assert len(set(ids)) == len(ids)


def test_no_case_contradicts_its_cell():
    for c in R.CASES + R.SLAB_CASES:
        assert R.route_case(c) == c.plan, (R.case_id(c), R.route_case(c), c.plan)
        p = c.plan
        assert (p.combine == R.NONE) == (p.ks == 1), c
        assert (c.norm and c.mode != R.F32R and c.epi != R.GELU) or not c.norm, c


def test_ragged_case_in_every_cell_that_admits_one():
    """Rows off the row tile in every cell; columns off 16 wherever the kernel takes such an N (the stream kernel wants whole panels,
    the gate / up pair 32-column groups, k-parts on the wide kernel N == 16384, the 4-wide reduce and the pair hand-off N % 256 == 0)."""
    by_cell = {}
    for c in R.CASES:
        by_cell.setdefault(R.cell_of(c), []).append(c)
    for cell, cs in by_cell.items():
        row_tile = {R.SKINNY: 16, R.MID: 16 * cell.mt, R.WIDE: 16 * cell.mt, R.STREAM: 16 * cell.mt, R.RING: 32 * max(cell.mt, 1),
                    R.TILE: 128, R.PP: 256}[cell.klass]
        assert any(c.M % row_tile for c in cs), cell
        whole_n = (cell.klass == R.STREAM or cell.epi == R.SILU or cell.combine in (R.REDUCE4, R.PP_PAIR) or
                   (cell.klass == R.WIDE and cell.combine != R.NONE))
        if cell in R.EXTRA_CELLS:
            continue
        assert whole_n or any(c.N % 16 for c in cs), cell


def test_old_tables_are_kept():
    """Every tuple of the two parity tables of tests/test_gpu_parity.py is in the case table, in order."""
    src = open(os.path.join(ROOT, "tests", "test_gpu_parity.py")).read()
    import re
    t1 = src.split("def test_gemm_kernels")[0].rsplit("@pytest.mark.parametrize", 1)[1]
    tuples = [tuple(eval(x)) for x in re.findall(r"\(\d+, \d+, \d+, \d, \d, (?:True|False)\)", t1)]
    assert len(tuples) == 34
    assert tuples == [(c.M, c.N, c.K, c.epi, int(c.mode != R.F16), c.mode == R.F32R) for c in R.OLD_KERNEL_CASES]
    t2 = src.split("def test_gemm_fused_rmsnorm")[0].rsplit("@pytest.mark.parametrize", 1)[1]
    tuples = [tuple(eval(x)) for x in re.findall(r"\(\d+, \d+, \d+, \d\)", t2)]
    assert tuples == [(c.M, c.N, c.K, c.epi) for c in R.OLD_NORM_CASES] and all(c.norm and c.mode == R.F16 for c in R.OLD_NORM_CASES)


def test_restatement_on_the_old_tuples():
    """What the older comments said of these tuples and what the launcher's rules give (the comments are corrected now)."""
    # 260 tiles, R = 4, K = 1024: 4 parts would save 36 x 0.75 = 27 us of a tile time against 30 us of slabs + reduce: no split
    assert R.route(1280, 13312, 1024, R.SILU, R.F16) == R.Plan(R.PP, 0, 0, 0, 0, 0, 1, R.NONE)
    # 12 x 64 = 768 tiles are three full rounds: no tail
    assert R.route(3072, 16384, 3072, R.SILU, R.F16) == R.Plan(R.PP, 0, 0, 0, 0, 0, 1, R.NONE)
    # K = 448 has 7 k-tiles, 7 / 4 = 1 part
    assert R.route(3000, 8192, 448, R.SILU, R.F16) == R.Plan(R.PP, 0, 0, 0, 0, 0, 1, R.NONE)
    # so no older kernel test reached the gate / up pair hand-off or pp_tail_reduce_kernel<EPI_SILU_GU16>; the table does now
    old = R.OLD_KERNEL_CASES + R.OLD_NORM_CASES
    assert not [c for c in old if c.epi == R.SILU and c.plan.klass == R.PP and c.plan.ks > 1]
    new = {(c.plan.combine, c.plan.ks >= 3) for c in R.NEW_CASES if c.epi == R.SILU and c.plan.klass == R.PP}
    assert (R.PP_PAIR, False) in new and (R.PP_REDUCE, True) in new
    # "skinny (M <= 16)": the skinny kernel takes 4 rows at the most, 5 and 16 rows with the norm fused are gemm_mid_kernel<2, ., NORM>
    assert R.route(5, 512, 1024, R.SILU, R.F16, norm=True)[:2] == (R.MID, 2) and R.route(16, 96, 320, R.PLAIN, R.F16, norm=True)[:2] == (R.MID, 2)
    # the lm_head output mode (fp32 without a residual) and the skinny kernel without LDS-staged activations were in neither table
    assert not [c for c in old if c.mode == R.F32] and not [c for c in old if c.plan.klass == R.SKINNY and not c.plan.alds]
    assert max(c.M * c.K * 2 for c in old if c.plan.klass == R.SKINNY) <= 64 * 1024


def test_stream_plan_against_the_shapes_the_source_names():
    """gemm_stream.hip's comments: wo / down at 4096 columns on one panel x the whole K; down at > 16 rows as 4 panels x 4 k-parts
    (fragment-ordered A); QKV as 3 panels x 2 k-parts (slabs); 320 panels as 5 x 4."""
    assert R.stream_plan(32, 4096, 4096, False, False) == (1, 1)
    assert R.stream_plan(40, 4096, 14336, False, True) == (4, 4) and R.stream_plan(17, 4096, 14336, False, True) == (1, 1)
    assert R.stream_plan(64, 6144, 4096, True, False) == (3, 2)
    assert R.stream_plan(48, 5120, 13824, False, True) == (5, 4) and R.stream_plan(64, 5120, 5120, False, True) is None
    assert R.stream_plan(8, 4096, 14336, False, False) == (1, 1) and R.stream_plan(40, 4096, 14336, False, False) is None


@pytest.mark.parametrize("c", [c for c in R.CASES + R.SLAB_CASES if not c.norm], ids=R.case_id)
def test_exact_family_is_exact(c):
    """From the reference alone: the largest |partial sum| any order can reach stays below 2^24 units, the scaled integers are exact
    in fp16 and bf16, and the GELU / gate-up pre-activations stay within PRE_RANGE (on a sample of rows for the large cases)."""
    assert R.exact_bound(c.K) < 1 << 24
    e = R.scale_exp(c.K)
    assert 0 < e <= 12                                              # 7 x 2^-12 is a normal fp16 number
    if c.M * c.N * c.K > 1 << 28 and c.epi == R.PLAIN:
        return                                                      # (the bound above does not depend on the values)
    A, W, bias, res, e2 = R.exact_inputs(c)
    assert e2 == e and A.abs().min() >= 1 and A.abs().max() <= R.A_MAX and W.abs().min() >= 1 and W.abs().max() <= R.W_MAX
    assert bias.abs().max() <= R.B_MAX and (res is None or res.abs().max() <= R.B_MAX)
    for dt in (torch.float16, torch.bfloat16):
        w = (W[:64].float() * 2.0 ** -e).to(dt)
        assert torch.equal(w.double(), W[:64].double() * 2.0 ** -e) and torch.equal(A[:64].to(dt).double(), A[:64].double())
    rows = torch.arange(c.M) if c.M * c.N * c.K <= 1 << 28 else torch.cat([torch.arange(8), torch.arange(c.M - 8, c.M)])
    a, w = A[rows].float(), W.float()
    worst = (a.abs() @ w.abs().T).max().item() + 2 * R.B_MAX
    assert worst <= R.exact_bound(c.K)
    pre = (a @ w.T + bias.float()) * 2.0 ** -e                      # (exact in fp32, by the bound above)
    if c.epi != R.PLAIN:
        assert pre.abs().max().item() <= R.PRE_RANGE, pre.abs().max().item()
        assert R.activate(pre, c.epi).abs().max().item() < 1024.0    # far inside fp16
    else:
        assert pre.abs().max().item() + 2 * R.B_MAX * 2.0 ** -e < 60000.0


def test_header_and_binding_know_the_plan_entry():
    from opus_pllm_amd import _cabi
    header = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    assert "int opus_debug_gemm_plan(opus_ctx *ctx, int32_t *plan);" in header
    lib = _cabi.lib()
    w = (__import__("ctypes").c_int32 * 8)()
    assert lib.opus_debug_gemm_plan(None, w) == -1
