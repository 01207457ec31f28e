"""The pure-Python HDF5 subset (utils/hdf5.py) against the HDF5 C library, and the Keras config
parser (model/keras_format.py) on known graphs.  CPU only; tests that need libhdf5 skip when
ctypes cannot load it."""
import copy
import importlib.util
import json
import subprocess
import time
import zipfile

import numpy as np
import pytest

from conftest import GOLDEN
from leaffliction_amd.model import keras_format as K
from leaffliction_amd.utils import hdf5

_spec = importlib.util.spec_from_file_location("make_golden_keras", GOLDEN / "make_golden_keras.py")
MK = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MK)

needs_lib = pytest.mark.skipif(MK.find_libhdf5() is None, reason="libhdf5 cannot be loaded through ctypes")

DTYPES = ["f4", "f8", "i1", "i2", "i4", "i8", "u1", "u2", "u4", "u8"]
PRESETS = {"tiny": ([16, 32, 64], 0.10, 0.30), "small": ([32, 64, 128], 0.15, 0.35),
           "base": ([32, 64, 128, 256], 0.15, 0.40)}


def _values(dt, shape, rng):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return rng.standard_normal(shape).astype(dt)
    info = np.iinfo(dt)
    return rng.randint(max(info.min, -2 ** 31), min(info.max, 2 ** 31 - 1), size=shape).astype(dt)


def _sample_tree(rng):
    flat = {}
    for i, dt in enumerate(DTYPES):
        flat[f"types/{dt}/scalar"] = _values(dt, (), rng)
        flat[f"types/{dt}/empty"] = np.zeros((0, 3), dt)
        flat[f"types/{dt}/rank{i % 4 + 1}"] = _values(dt, (3, 2, 4, 5)[:i % 4 + 1], rng)
    flat["deep/a/b/c/d/leaf"] = np.arange(7, dtype=np.float32)
    flat["empty_group"] = None
    return flat


@needs_lib
def test_reader_matches_libhdf5_files(tmp_path):
    rng = np.random.RandomState(0)
    flat = _sample_tree(rng)
    for i in range(500):                                    # > 8 * 32 entries: a two-level group B-tree
        flat[f"wide/m{i:03d}"] = np.array([i], np.int32)
    flat["layout/compact"] = _values("f4", (4, 5), rng)
    flat["layout/chunked"] = _values("f8", (7, 9, 3), rng)    # edge chunks in every dimension
    flat["layout/chunked_i2"] = _values("i2", (10,), rng)
    layout = {"layout/compact": ("compact",), "layout/chunked": ("chunked", (3, 4, 2)),
              "layout/chunked_i2": ("chunked", (4,))}
    MK.H5Lib().write(tmp_path / "lib.h5", flat, layout)
    got = hdf5.read(tmp_path / "lib.h5")
    want = {k: v for k, v in flat.items() if v is not None}
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, k
        assert np.array_equal(got[k], v), k
    walk = {p: (g, d) for p, g, d in hdf5.walk(tmp_path / "lib.h5")}
    assert walk["empty_group"] == ([], [])
    assert len(walk["wide"][1]) == 500


@needs_lib
def test_writer_files_read_by_libhdf5(tmp_path):
    rng = np.random.RandomState(1)
    flat = _sample_tree(rng)
    for i in range(300):
        flat[f"wide/m{i:03d}"] = np.array([i, -i], np.int64)
    hdf5.write(tmp_path / "ours.h5", hdf5.nest({k: ({} if v is None else v) for k, v in flat.items()}))
    lib = MK.H5Lib()
    for k, v in flat.items():
        if v is not None:
            got = lib.read(tmp_path / "ours.h5", k, v.dtype)
            assert got.shape == v.shape and np.array_equal(got, v), k
    h5dump = MK.find_h5dump()
    if h5dump:
        p = subprocess.run([h5dump, str(tmp_path / "ours.h5")], capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert hdf5.read(tmp_path / "ours.h5").keys() == {k for k, v in flat.items() if v is not None}


def test_writer_round_trip_without_libhdf5():
    rng = np.random.RandomState(2)
    flat = {k: v for k, v in _sample_tree(rng).items() if v is not None}
    data = hdf5.write(None, hdf5.nest(flat))
    got = hdf5.read(data)
    assert sorted(got) == sorted(flat)
    assert all(np.array_equal(got[k], v) and got[k].dtype == v.dtype for k, v in flat.items())


def _damaged_files():
    arch = zipfile.ZipFile(GOLDEN / "keras_tiny32.keras")
    lib_file = arch.read("model.weights.h5")
    ours = hdf5.write(None, hdf5.nest({k: v for k, v in _sample_tree(np.random.RandomState(3)).items()
                                       if v is not None}))
    return [("libhdf5", lib_file), ("ours", ours)]


@pytest.mark.parametrize("which", [0, 1])
def test_truncated_files_raise_value_error(which):
    name, data = _damaged_files()[which]
    t0 = time.time()
    for cut in range(0, len(data), 97):
        with pytest.raises(ValueError):
            hdf5.read(data[:cut])
    assert time.time() - t0 < 120, name


@pytest.mark.parametrize("which", [0, 1])
def test_flipped_header_bytes_raise_value_error_or_read(which):
    """Random bytes flipped in the first 4 KB (superblock, root group, first B-tree nodes): the
    reader either still reads the file or raises ValueError, quickly, and never anything else."""
    name, data = _damaged_files()[which]
    rng = np.random.RandomState(4 + which)
    t0, raised = time.time(), 0
    for _ in range(300):
        b = bytearray(data)
        for pos in rng.randint(0, min(4096, len(b)), size=rng.randint(1, 4)):
            b[pos] ^= int(rng.randint(1, 256))
        try:
            hdf5.read(bytes(b))
        except ValueError:
            raised += 1
    assert time.time() - t0 < 180, name
    assert raised > 30, f"{name}: only {raised} of 300 damaged files were refused"


def test_outside_subset_is_refused():
    with pytest.raises(ValueError, match="signature"):
        hdf5.read(b"not an hdf5 file at all" * 40)
    with pytest.raises(ValueError, match="outside the supported subset"):
        hdf5.write(None, {"c": np.zeros(2, np.complex64)})


# ------------------------------------------------------------------ keras config
def _hp(preset, use_norm, **kw):
    widths, db, dt = PRESETS[preset]
    hp = dict(num_classes=7, img_size=64, widths=widths, use_norm=use_norm, use_se=True, augment=True,
              drop_block=db, drop_top=dt, l2_reg=0.0)
    hp.update(kw)
    return hp


@pytest.mark.parametrize("preset", sorted(PRESETS))
@pytest.mark.parametrize("use_norm", [True, False])
def test_parse_config_known_answers(preset, use_norm):
    hp = _hp(preset, use_norm)
    got, src = K.parse_config(K.functional_config(hp))
    assert got == hp
    assert sorted(src) == sorted(n for n, _s in K.keras_shapes(hp))


def test_parse_config_variants():
    hp = _hp("tiny", True, use_se=False, augment=False, drop_block=0.0, drop_top=0.0, l2_reg=1e-4,
             num_classes=3, img_size=48)
    cfg = K.functional_config(hp)
    assert K.parse_config(cfg)[0] == hp
    legacy = copy.deepcopy(cfg)                 # Keras 2 style: list-form nodes, batch_input_shape, Policy
    for L in legacy["config"]["layers"]:
        if L["inbound_nodes"]:
            L["inbound_nodes"] = [[[n, 0, 0, {}] for n in K._inbound(L, L["name"])]]
        if L["class_name"] == "InputLayer":
            L["config"]["batch_input_shape"] = L["config"].pop("batch_shape")
        else:
            L["config"]["dtype"] = {"class_name": "Policy", "config": {"name": "mixed_float16"}}
    assert K.parse_config(legacy)[0] == hp
    renamed = json.loads(json.dumps(cfg).replace('"conv2d', '"conv2d_x'))
    assert K.parse_config(renamed)[0] == hp


def _mutate(cfg, cls, index, fn):
    cfg = copy.deepcopy(cfg)
    layer = [L for L in cfg["config"]["layers"] if L["class_name"] == cls][index]
    fn(layer)
    return cfg, layer["name"]


@pytest.mark.parametrize("case", ["separable", "bn_eps", "se_ratio", "unknown", "stride"])
def test_parse_config_refusals(case):
    cfg = K.functional_config(_hp("small", True))
    if case == "separable":
        cfg, name = _mutate(cfg, "Conv2D", 1, lambda L: L.update(class_name="SeparableConv2D"))
        match = "SeparableConv2D"
    elif case == "bn_eps":
        cfg, name = _mutate(cfg, "BatchNormalization", 2, lambda L: L["config"].update(epsilon=1e-5))
        match = "epsilon"
    elif case == "se_ratio":
        se1 = [L for L in cfg["config"]["layers"] if L["class_name"] == "Conv2D"
               and L["config"]["kernel_size"] == [1, 1] and L["config"]["activation"] == "relu"][0]
        se1["config"]["filters"] = se1["config"]["filters"] * 2
        name, match = se1["name"], "ratio"
    elif case == "unknown":
        cfg, name = _mutate(cfg, "Activation", 3, lambda L: L.update(class_name="LeakyReLU"))
        match = "LeakyReLU"
    else:
        cfg, name = _mutate(cfg, "Conv2D", 0, lambda L: L["config"].update(strides=[2, 2]))
        match = "strides"
    with pytest.raises(ValueError, match=match) as e:
        K.parse_config(cfg)
    assert name in str(e.value)


def test_weight_shape_mismatch_is_refused(tmp_path):
    hp = _hp("tiny", True, img_size=32)
    names = [n for n, _s in K.keras_shapes(hp)]
    arrays = [np.ones(s, np.float32) for _n, s in K.keras_shapes(hp)]
    K.write_archive(tmp_path / "m.keras", hp, names, arrays)
    with zipfile.ZipFile(tmp_path / "m.keras") as z:
        cfg = json.loads(z.read("config.json"))
        h5 = hdf5.read(z.read("model.weights.h5"))
    key = next(k for k in h5 if k.startswith("layers/dense/vars/0"))
    h5[key] = np.ones((3, 3), np.float32)
    with pytest.raises(ValueError, match="shape"):
        K.weights_from_h5(cfg, h5)


def test_keras_archive_round_trip_on_host(tmp_path):
    for preset in PRESETS:
        hp = _hp(preset, preset != "small", img_size=32)
        rng = np.random.RandomState(5)
        names = [n for n, _s in K.keras_shapes(hp)]
        arrays = [rng.standard_normal(s).astype(np.float32) for _n, s in K.keras_shapes(hp)]
        K.write_archive(tmp_path / f"{preset}.keras", hp, names, arrays)
        hp2, names2, arrays2 = K.read_archive(tmp_path / f"{preset}.keras")
        assert hp2 == hp and names2 == names
        assert all(np.array_equal(a, b) for a, b in zip(arrays, arrays2))
        with zipfile.ZipFile(tmp_path / f"{preset}.keras") as z:
            meta = json.loads(z.read("metadata.json"))
            assert meta["keras_version"] == K.KERAS_VERSION and "compile_config" not in json.loads(z.read("config.json"))
            h5 = hdf5.walk(z.read("model.weights.h5"))
        groups = {p for p, _g, _d in h5}
        assert "layers/input_layer/vars" in groups and "vars" in groups


def test_libhdf5_fixture_reads_on_host():
    """The committed fixture (weights written by libhdf5, mixed_float16, counter-suffixed names)."""
    hp, names, arrays = K.read_archive(GOLDEN / "keras_tiny32.keras")
    ref = np.load(GOLDEN / "keras_tiny32.npz")
    assert hp == json.loads(str(ref["hp"]))
    keys = sorted(k for k in ref.files if k != "hp")
    assert [k.split(":", 1)[1] for k in keys] == names
    assert all(np.array_equal(ref[k], a) and a.dtype == np.float32 for k, a in zip(keys, arrays))
