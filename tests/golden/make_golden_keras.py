"""Writes tests/golden/keras_tiny32.keras and keras_tiny32.npz: a Keras-layout leaf_cnn archive
whose model.weights.h5 is written by the HDF5 C library itself (through ctypes, default property
lists, as h5py uses them), and the arrays it holds in get_weights() order.

The model is the `tiny` preset (widths 16/32/64, spatial dropout 0.10, top dropout 0.30) at
img_size 32 with 5 classes, normalization and augmentation on.  Its config.json is the graph
`keras_format.functional_config` describes, rewritten the way a long Keras session would save it:
counter-suffixed layer names (conv2d_17, ...), a `mixed_float16` DTypePolicy on every layer and
dict-form inbound_nodes.  The weights file also carries an `optimizer/` group, and its `layers`
group (one member per layer) is far wider than libhdf5's default of 8 entries per symbol node,
so the reader walks a multi-node B-tree.

This module doubles as the tests' libhdf5 binding (`H5Lib`); it needs libhdf5 only when run.
Run from the repository root:  python tests/golden/make_golden_keras.py
"""
from __future__ import annotations

import ctypes as C
import ctypes.util
import io
import json
import os
import shutil
import sys
import zipfile
from pathlib import Path
from typing import Dict, Optional

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
GOLDEN = Path(__file__).resolve().parent
HP = dict(num_classes=5, img_size=32, widths=[16, 32, 64], use_norm=True, use_se=True, augment=True,
          drop_block=0.10, drop_top=0.30, l2_reg=0.0)
MIXED = {"module": "keras", "class_name": "DTypePolicy", "config": {"name": "mixed_float16"},
         "registered_name": None}
UID_OFFSET = 17                 # the session had already built layers of every class 17 times

hid_t = C.c_int64
H5P_DEFAULT, H5S_ALL, H5F_ACC_RDONLY, H5F_ACC_TRUNC = 0, 0, 0, 2
H5D_COMPACT, H5D_CONTIGUOUS, H5D_CHUNKED = 0, 1, 2
_TYPES = {"f4": "H5T_IEEE_F32LE_g", "f8": "H5T_IEEE_F64LE_g", "i1": "H5T_STD_I8LE_g", "i2": "H5T_STD_I16LE_g",
          "i4": "H5T_STD_I32LE_g", "i8": "H5T_STD_I64LE_g", "u1": "H5T_STD_U8LE_g", "u2": "H5T_STD_U16LE_g",
          "u4": "H5T_STD_U32LE_g", "u8": "H5T_STD_U64LE_g"}


def find_libhdf5() -> Optional[str]:
    """The HDF5 C library, if the machine has one: LEAFFLICTION_LIBHDF5, the linker's search path,
    then the lib/ beside h5dump or under the usual conda / local prefixes."""
    cands = [os.environ.get("LEAFFLICTION_LIBHDF5"), ctypes.util.find_library("hdf5")]
    h5dump = shutil.which("h5dump")
    for prefix in ([Path(h5dump).resolve().parent.parent] if h5dump else []) + \
            [Path(p) for p in (os.environ.get("CONDA_PREFIX"), sys.prefix, "/opt/conda", "/usr/local") if p]:
        cands += sorted(str(p) for p in (prefix / "lib").glob("libhdf5.so*"))
    for c in cands:
        if c:
            try:
                C.CDLL(c)
                return c
            except OSError:
                continue
    return None


def find_h5dump() -> Optional[str]:
    lib = find_libhdf5()
    for c in (shutil.which("h5dump"), lib and str(Path(lib).resolve().parent.parent / "bin" / "h5dump")):
        if c and Path(c).is_file():
            return c
    return None


class H5Lib:
    def __init__(self, path: Optional[str] = None) -> None:
        path = path or find_libhdf5()
        if path is None:
            raise OSError("libhdf5 not found")
        L = self.L = C.CDLL(path)
        for fn in ("H5Fcreate", "H5Fopen", "H5Gcreate2", "H5Screate", "H5Screate_simple", "H5Dcreate2",
                   "H5Dopen2", "H5Dget_space", "H5Dget_type", "H5Pcreate"):
            getattr(L, fn).restype = hid_t
        L.H5Fcreate.argtypes = [C.c_char_p, C.c_uint, hid_t, hid_t]
        L.H5Fopen.argtypes = [C.c_char_p, C.c_uint, hid_t]
        L.H5Gcreate2.argtypes = [hid_t, C.c_char_p, hid_t, hid_t, hid_t]
        L.H5Screate.argtypes = [C.c_int]
        L.H5Screate_simple.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.c_void_p]
        L.H5Dcreate2.argtypes = [hid_t, C.c_char_p, hid_t, hid_t, hid_t, hid_t, hid_t]
        L.H5Dopen2.argtypes = [hid_t, C.c_char_p, hid_t]
        L.H5Dwrite.argtypes = [hid_t, hid_t, hid_t, hid_t, hid_t, C.c_void_p]
        L.H5Dread.argtypes = [hid_t, hid_t, hid_t, hid_t, hid_t, C.c_void_p]
        L.H5Dget_space.argtypes = L.H5Dget_type.argtypes = [hid_t]
        L.H5Sget_simple_extent_ndims.argtypes = [hid_t]
        L.H5Sget_simple_extent_dims.argtypes = [hid_t, C.POINTER(C.c_uint64), C.c_void_p]
        L.H5Pcreate.argtypes = [hid_t]
        L.H5Pset_layout.argtypes = [hid_t, C.c_int]
        L.H5Pset_chunk.argtypes = [hid_t, C.c_int, C.POINTER(C.c_uint64)]
        L.H5Tequal.argtypes = [hid_t, hid_t]
        for fn in ("H5Fclose", "H5Gclose", "H5Sclose", "H5Dclose", "H5Pclose", "H5Tclose"):
            getattr(L, fn).argtypes = [hid_t]
        if L.H5open() < 0:
            raise OSError("H5open failed")
        self.types = {k: hid_t.in_dll(L, v).value for k, v in _TYPES.items()}
        self.dcpl_class = hid_t.in_dll(L, "H5P_CLS_DATASET_CREATE_ID_g").value

    @staticmethod
    def _ok(v: int, what: str) -> int:
        if v < 0:
            raise RuntimeError(f"libhdf5: {what} failed")
        return v

    def _type(self, dt: np.dtype) -> int:
        return self.types[f"{dt.kind}{dt.itemsize}"]

    def write(self, path, flat: Dict[str, Optional[np.ndarray]], layout: Dict[str, tuple] = None) -> None:
        """{"a/b": array, "g": None (empty group)} -> an HDF5 file written by libhdf5.  `layout` maps a
        dataset path to ("compact",) or ("chunked", chunk_dims); contiguous otherwise."""
        L = self.L
        layout = layout or {}
        f = self._ok(L.H5Fcreate(str(path).encode(), H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT), "H5Fcreate")
        groups: Dict[str, int] = {"": f}
        try:
            for key in flat:
                parts = key.split("/")
                for i in range(1, len(parts) + (flat[key] is None)):
                    g = "/".join(parts[:i])
                    if g not in groups:
                        groups[g] = self._ok(L.H5Gcreate2(groups["/".join(parts[:i - 1])], parts[i - 1].encode(),
                                                          H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), f"H5Gcreate2 {g}")
                arr = flat[key]
                if arr is None:
                    continue
                arr = np.ascontiguousarray(arr).reshape(np.shape(arr))
                if arr.ndim == 0:
                    space = L.H5Screate(0)
                else:
                    space = L.H5Screate_simple(arr.ndim, (C.c_uint64 * arr.ndim)(*arr.shape), None)
                self._ok(space, f"dataspace for {key}")
                dcpl = H5P_DEFAULT
                spec = layout.get(key)
                if spec:
                    dcpl = self._ok(L.H5Pcreate(self.dcpl_class), "H5Pcreate")
                    if spec[0] == "compact":
                        self._ok(L.H5Pset_layout(dcpl, H5D_COMPACT), "H5Pset_layout")
                    else:
                        self._ok(L.H5Pset_chunk(dcpl, arr.ndim, (C.c_uint64 * arr.ndim)(*spec[1])), "H5Pset_chunk")
                t = self._type(arr.dtype)
                d = self._ok(L.H5Dcreate2(groups["/".join(parts[:-1])], parts[-1].encode(), t, space,
                                          H5P_DEFAULT, dcpl, H5P_DEFAULT), f"H5Dcreate2 {key}")
                if arr.size:
                    self._ok(L.H5Dwrite(d, t, H5S_ALL, H5S_ALL, H5P_DEFAULT, arr.ctypes.data), f"H5Dwrite {key}")
                L.H5Dclose(d)
                L.H5Sclose(space)
                if dcpl != H5P_DEFAULT:
                    L.H5Pclose(dcpl)
        finally:
            for g, gid in groups.items():
                if g:
                    L.H5Gclose(gid)
            L.H5Fclose(f)

    def read(self, path, key: str, dtype) -> np.ndarray:
        """One dataset through H5Dread, checking that its stored type is `dtype`'s."""
        L = self.L
        dtype = np.dtype(dtype)
        f = self._ok(L.H5Fopen(str(path).encode(), H5F_ACC_RDONLY, H5P_DEFAULT), "H5Fopen")
        try:
            d = self._ok(L.H5Dopen2(f, ("/" + key).encode(), H5P_DEFAULT), f"H5Dopen2 {key}")
            space, ftype = L.H5Dget_space(d), L.H5Dget_type(d)
            rank = L.H5Sget_simple_extent_ndims(space)
            dims = (C.c_uint64 * max(rank, 1))()
            L.H5Sget_simple_extent_dims(space, dims, None)
            same = L.H5Tequal(ftype, self._type(dtype)) > 0
            out = np.zeros(tuple(dims[:rank]), dtype)
            if out.size:
                self._ok(L.H5Dread(d, self._type(dtype), H5S_ALL, H5S_ALL, H5P_DEFAULT, out.ctypes.data), "H5Dread")
            L.H5Tclose(ftype)
            L.H5Sclose(space)
            L.H5Dclose(d)
        finally:
            L.H5Fclose(f)
        if not same:
            raise AssertionError(f"{key}: stored type differs from {dtype}")
        return out


# ----------------------------------------------------------------- the fixture
def _session_config(hp) -> dict:
    """functional_config(hp) as a long-running session would save it (see the module docstring)."""
    from leaffliction_amd.model.keras_format import functional_config
    cfg = functional_config(hp)
    layers = cfg["config"]["layers"]
    rename = {}
    for L in layers:
        n = L["name"]
        if n in ("augment", "input_norm"):
            continue
        base, _, k = n.rpartition("_")
        base, k = (base, int(k)) if k.isdigit() and base else (n, 0)
        rename[n] = f"{base}_{k + UID_OFFSET}"

    def fix(o):
        if isinstance(o, dict):
            for key, v in o.items():
                if key == "keras_history":
                    v[0] = rename.get(v[0], v[0])
                elif key == "name" and isinstance(v, str):
                    o[key] = rename.get(v, v)
                else:
                    fix(v)
        elif isinstance(o, list):
            for v in o:
                fix(v)

    for L in layers:
        fix(L)
        if L["class_name"] != "InputLayer":
            L["config"]["dtype"] = dict(MIXED)
    for key in ("input_layers", "output_layers"):
        cfg["config"][key][0] = rename[cfg["config"][key][0]]
    return cfg


def _flatten(tree: dict, prefix: str = "") -> Dict[str, Optional[np.ndarray]]:
    out: Dict[str, Optional[np.ndarray]] = {}
    for k, v in tree.items():
        p = f"{prefix}/{k}" if prefix else k
        if isinstance(v, dict):
            sub = _flatten(v, p)
            out.update(sub if sub else {p: None})
        else:
            out[p] = v
    return out


def main() -> None:
    sys.path.insert(0, str(ROOT))
    from leaffliction_amd.model.keras_format import keras_shapes, weights_tree
    rng = np.random.RandomState(20261015)
    names, arrays = [], []
    for name, shape in keras_shapes(HP):
        a = rng.standard_normal(shape).astype(np.float32) * np.float32(0.2)
        if name.endswith(("variance", ".gamma")):
            a = (np.abs(a) + np.float32(0.5)).astype(np.float32)
        names.append(name)
        arrays.append(a)
    cfg = _session_config(HP)
    tree = weights_tree(cfg, HP, names, arrays)
    tree["optimizer"] = {"vars": {"0": np.array(1234, np.int64), "1": np.float32(1e-3) * np.ones((), np.float32),
                                  "2": rng.standard_normal((3, 3, 3, 16)).astype(np.float32)}}
    h5_path = GOLDEN / "_keras_tiny32_weights.h5"
    H5Lib().write(h5_path, _flatten(tree))
    h5 = h5_path.read_bytes()
    h5_path.unlink()
    with zipfile.ZipFile(GOLDEN / "keras_tiny32.keras", "w", zipfile.ZIP_STORED) as z:
        z.writestr("metadata.json", json.dumps({"keras_version": "3.3.3", "date_saved": "2026-10-15@12:00:00"}))
        z.writestr("config.json", json.dumps(cfg))
        z.writestr("model.weights.h5", h5)
    buf = io.BytesIO()
    np.savez(buf, hp=np.array(json.dumps(HP)), **{f"{i:03d}:{n}": a for i, (n, a) in enumerate(zip(names, arrays))})
    (GOLDEN / "keras_tiny32.npz").write_bytes(buf.getvalue())
    print(f"keras_tiny32.keras ({len(h5)}-byte weights file), keras_tiny32.npz: {len(names)} arrays")


if __name__ == "__main__":
    main()
