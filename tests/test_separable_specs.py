"""What the separable leaf_cnn needs that can be checked without a GPU: the depthwise entry points refuse bad
arguments on the host, and the parameter list of `separable=True` is Keras' (depthwise_kernel, pointwise_kernel)."""
from leaffliction_amd import _lib
from leaffliction_amd.model.cnn import _specs, _weight_names


def test_depthwise_entry_points_check_their_arguments_on_the_host():
    lib = _lib.load()
    assert lib.lf_dwconv3x3_f32(None, None, None, 1, 3, 4, 4, None, None, 0, None) == -1
    assert b"lf_dwconv3x3_f32" in lib.lf_last_error() and b"null" in lib.lf_last_error()
    assert lib.lf_dwconv3x3_bwd_f32(None, None, None, None, 0, None, 1, 3, 4, 4, None, None, 0, None, 0, None) == -1
    assert b"lf_dwconv3x3_bwd_f32" in lib.lf_last_error() and b"null" in lib.lf_last_error()
    # nine floats per lane and unit: at least one unit per plane and column group
    assert lib.lf_dwconv3x3_bwd_workspace(2, 3, 5, 7) >= 2 * 3 * 7 * 9 * 4
    assert lib.lf_dwconv3x3_bwd_workspace(256, 32, 224, 224) <= 1 << 27
    assert lib.lf_dwconv3x3_bwd_workspace(2, 0, 5, 7) == 0


def test_separable_specs_split_every_block_conv_and_nothing_else():
    dense = _specs(4, [16, 32], True)
    sep = _specs(4, [16, 32], True, separable=True)
    assert dense == _specs(4, [16, 32], True, separable=False)
    assert [s for s in dense if s[2] != "w3"] == [s for s in sep if s[2] not in ("dw", "pw")]
    convs = [(n, s) for n, s, k in dense if k == "w3"]
    pairs = [(n, s, k) for n, s, k in sep if k in ("dw", "pw")]
    assert len(pairs) == 2 * len(convs) == 10
    for i, (name, (cin, taps, cout)) in enumerate(convs):
        assert taps == 9
        assert pairs[2 * i] == (name[:-2] + ".dw", (cin, 9), "dw")
        assert pairs[2 * i + 1] == (name[:-2] + ".pw", (cin, 1, cout), "pw")
    names = _weight_names(sep, True)
    assert names[:5] == ["input_norm.mean", "input_norm.variance", "stem.dw", "stem.pw", "stem.bn.gamma"]
    assert all(n.startswith(("stem.", "s0.", "s1.", "dense.", "input_norm.")) for n in names)
