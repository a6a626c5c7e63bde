"""The loader's table of quantised decoder-weight formats (weights.WEIGHT_FORMATS): its suffixes and dtype codes, the tensors it
applies to, and the keywords it accepts.  No GPU."""
import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, weights


def test_every_format_names_two_suffixes_with_existing_distinct_dtype_codes():
    known = {_cabi.OPUS_F16, _cabi.OPUS_F32, _cabi.OPUS_I32, _cabi.OPUS_I64, _cabi.OPUS_U8, _cabi.OPUS_F8E4M3, _cabi.OPUS_I8,
             _cabi.OPUS_F4E2M1X2, _cabi.OPUS_E8M0}
    by_suffix = {}
    for f in weights.WEIGHT_FORMATS:
        assert len(f.suffixes) == 2 and callable(f.quantize)
        for sfx, code in f.suffixes:
            assert len(sfx) == 3 and sfx[0] == "." and sfx not in by_suffix, sfx      # (bind() looks the last three characters up)
            assert code in known and code not in (_cabi.OPUS_F16, _cabi.OPUS_F32), (sfx, code)
            by_suffix[sfx] = code
    assert len(set(by_suffix.values())) == len(by_suffix) == 2 * len(weights.WEIGHT_FORMATS)
    assert by_suffix == {".q8": _cabi.OPUS_F8E4M3, ".e8": _cabi.OPUS_I8, ".q4": _cabi.OPUS_F4E2M1X2, ".s4": _cabi.OPUS_E8M0}


def test_quantized_names_are_the_four_projections_of_every_decoder_layer():
    for cfg, mats in ((opa.micro(), ("wqkv", "wo", "wgu", "wd")), (opa.micro_opt(), ("wqkv", "wo", "w1", "w2"))):
        names = weights.quantized_names(cfg)
        assert names == [f"dec.{l}.{m}" for l in range(cfg.dec_layers) for m in mats]
        assert len(names) == len(set(names)) == 4 * cfg.dec_layers
        assert set(names) <= {f.name for f in weights.fused_spec(cfg)}


def test_keywords_of_the_table_are_the_accepted_formats():
    keywords = [k for f in weights.WEIGHT_FORMATS for k in (f.keyword, f.keyword_dequantized)]
    assert len(set(keywords)) == len(keywords)
    assert weights.DECODER_WEIGHT_FORMATS[0] is None and list(weights.DECODER_WEIGHT_FORMATS[1:]) == keywords
    assert all(f.keyword_dequantized == f.keyword + "_dequantized" for f in weights.WEIGHT_FORMATS)
