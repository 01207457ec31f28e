"""Keras 3 `.keras` archives of leaf_cnn: `config.json` + `metadata.json` + `model.weights.h5`.

Reading walks the Functional graph in `config.json`, checks that it is the reference's leaf_cnn
(srcs/model/cnn.py: stem conv block, residual blocks with optional squeeze-and-excitation and a
1x1 projection where the width changes, spatial dropout + max-pool per stage, global pooling,
dropout, softmax dense) and recovers the `build_leafcnn` hyperparameters from it.  Layers are
identified by their place in the graph, never by their names (Keras numbers auto-named layers
per session).  Both `inbound_nodes` encodings (Keras 3 dicts, legacy lists), string or
`DTypePolicy` dtypes and `batch_shape` / `batch_input_shape` are accepted.

Weights follow Keras 3's `saving_lib` layout: the model's layers, in `config.json` order, are
stored under `layers/<snake_case class name>[_<n>]/vars/<i>` (the counter is per class within
the container), variables in trainable + non-trainable order.  Anything else in the file (the
augmentation layers' seed-generator state, `optimizer/`) is ignored on reading.

Writing does the reverse for a LeafCNN: a Functional config with the layer names a fresh Keras
session running `build_leafcnn` would assign, `metadata.json`, and a `model.weights.h5` holding
every variable Keras 3's loader looks for, including the InputLayer's empty group and the seed
generators' state.  No `compile_config`: the archive loads uncompiled.  Written against the
Keras 3.x `saving_lib` layout (KERAS_VERSION below); no Keras is available to confirm that
Keras itself opens the result.
"""
from __future__ import annotations

import datetime
import json
import re
import zipfile
from collections import defaultdict
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from ..utils import hdf5
from .cnn import BN_EPS, _specs, _weight_names

KERAS_VERSION = "3.3.3"
SE_RATIO = 8


def snake_case(name: str) -> str:
    """keras.src.utils.naming.to_snake_case: the prefix of auto names and of weight paths."""
    name = re.sub(r"\W+", "", name)
    name = re.sub("(.)([A-Z][a-z]+)", r"\1_\2", name)
    return re.sub("([a-z])([A-Z])", r"\1_\2", name).lower()


def keras_shapes(hp: Dict[str, Any]) -> List[Tuple[str, Tuple[int, ...]]]:
    """(weight name, Keras shape) in get_weights() order for the model `hp` describes."""
    specs = _specs(int(hp["num_classes"]), list(hp["widths"]), bool(hp["use_se"]))
    shape = {}
    for name, s, kind in specs:
        if kind == "w3" or (kind == "w1" and len(s) == 3):
            k = int(round(s[1] ** 0.5))
            shape[name] = (k, k, s[0], s[2])
        elif kind == "w1":
            shape[name] = (1, 1) + tuple(s)
        else:
            shape[name] = tuple(s)
        if name.endswith(".beta"):
            shape[name[:-5] + ".moving_mean"] = shape[name[:-5] + ".moving_variance"] = tuple(s)
    shape["input_norm.mean"] = shape["input_norm.variance"] = (3,)
    return [(n, shape[n]) for n in _weight_names(specs, bool(hp["use_norm"]))]


# ===================================================================== reading
def _refuse(layer: Optional[str], msg: str):
    raise ValueError(f"keras config: layer {layer!r}: {msg}" if layer else f"keras config: {msg}")


def _tensor_refs(obj) -> List[str]:
    """Layer names of the keras tensors in one Keras 3 node's args, in order."""
    if isinstance(obj, dict):
        if obj.get("class_name") == "__keras_tensor__":
            return [obj["config"]["keras_history"][0]]
        return [r for v in obj.values() for r in _tensor_refs(v)]
    if isinstance(obj, (list, tuple)):
        return [r for v in obj for r in _tensor_refs(v)]
    return []


def _inbound(layer: dict, name: str) -> List[str]:
    nodes = layer.get("inbound_nodes") or []
    if len(nodes) > 1:
        _refuse(name, f"called {len(nodes)} times (shared layers are not part of leaf_cnn)")
    if not nodes:
        return []
    node = nodes[0]
    if isinstance(node, dict):                                    # Keras 3: {"args": [...], "kwargs": {}}
        return _tensor_refs(node.get("args", []))
    if isinstance(node, list):                                    # legacy: [[name, node, tensor, kwargs], ...]
        if all(isinstance(e, list) and e and isinstance(e[0], str) for e in node):
            return [e[0] for e in node]
    _refuse(name, f"unreadable inbound_nodes entry {node!r:.80}")


def _dtype_ok(cfg: dict, name: str) -> None:
    d = cfg.get("dtype")
    if d is None or isinstance(d, str):
        return
    if isinstance(d, dict) and d.get("class_name") in ("DTypePolicy", "FloatDTypePolicy", "Policy") \
            and isinstance(d.get("config", {}).get("name"), str):
        return
    _refuse(name, f"unreadable dtype policy {d!r:.80}")


def _pair(v, what: str, name: str) -> Tuple[int, int]:
    if isinstance(v, int):
        return v, v
    if isinstance(v, (list, tuple)) and len(v) == 2:
        return int(v[0]), int(v[1])
    _refuse(name, f"{what} {v!r}")


def _l2_of(reg) -> float:
    if reg is None:
        return 0.0
    c = reg.get("config", {}) if isinstance(reg, dict) else {}
    if isinstance(reg, dict) and reg.get("class_name") in ("L2", "L1L2") and not c.get("l1", 0.0):
        return float(c.get("l2", 0.0))
    raise ValueError(f"kernel_regularizer {reg!r:.80} (only L2 is supported)")


class _Graph:
    def __init__(self, config: dict) -> None:
        if not isinstance(config, dict) or config.get("class_name") not in ("Functional", "Model"):
            _refuse(None, f"top-level class {config.get('class_name') if isinstance(config, dict) else config!r} "
                          "(a Functional model is expected)")
        self.layers: List[dict] = list(config.get("config", {}).get("layers") or [])
        self.order: List[str] = []
        self.by: Dict[str, dict] = {}
        for L in self.layers:
            name = L.get("name") or L.get("config", {}).get("name")
            if not isinstance(name, str) or name in self.by:
                _refuse(name, "missing or duplicate layer name")
            self.by[name] = L
            self.order.append(name)
        self.inputs = {n: _inbound(self.by[n], n) for n in self.order}
        self.users: Dict[str, List[str]] = defaultdict(list)
        for n in self.order:
            for src in self.inputs[n]:
                if src not in self.by:
                    _refuse(n, f"input from unknown layer {src!r}")
                self.users[src].append(n)
        for n in self.order:
            if self.cls(n) == "SeparableConv2D":
                _refuse(n, "SeparableConv2D: this backend has no depthwise-separable convolution")
            _dtype_ok(self.cfg(n), n)
        self.seen: set = set()

    def cls(self, n: str) -> str:
        return self.by[n].get("class_name", "")

    def cfg(self, n: str) -> dict:
        return self.by[n].get("config", {})

    def take(self, n: str, *classes: str) -> dict:
        if self.cls(n) not in classes:
            _refuse(n, f"{self.cls(n)} where leaf_cnn has {' or '.join(classes)}")
        self.seen.add(n)
        return self.cfg(n)

    def one_user(self, n: str) -> str:
        u = self.users.get(n, [])
        if len(u) != 1:
            _refuse(n, f"feeds {len(u)} layers ({u}) where leaf_cnn has one")
        return u[0]

    # -------------------------------------------------------------- layer kinds
    def conv(self, n: str, k: int, bias: bool, act: str) -> Tuple[int, float]:
        c = self.take(n, "Conv2D")
        if _pair(c.get("kernel_size"), "kernel_size", n) != (k, k):
            _refuse(n, f"kernel_size {c.get('kernel_size')} ({k}x{k} expected)")
        if _pair(c.get("strides", 1), "strides", n) != (1, 1) or \
                _pair(c.get("dilation_rate", 1), "dilation_rate", n) != (1, 1) or c.get("groups", 1) != 1:
            _refuse(n, "strides / dilation / groups other than 1")
        if k > 1 and c.get("padding") != "same":
            _refuse(n, f"padding {c.get('padding')!r} ('same' expected)")
        if c.get("data_format") not in (None, "channels_last"):
            _refuse(n, f"data_format {c.get('data_format')!r}")
        if bool(c.get("use_bias", True)) != bias:
            _refuse(n, f"use_bias={c.get('use_bias', True)} (leaf_cnn has {bias})")
        if (c.get("activation") or "linear") != act:
            _refuse(n, f"activation {c.get('activation')!r} ({act!r} expected)")
        try:
            l2 = _l2_of(c.get("kernel_regularizer"))
        except ValueError as e:
            _refuse(n, str(e))
        return int(c["filters"]), l2

    def bn(self, n: str) -> None:
        c = self.take(n, "BatchNormalization")
        if abs(float(c.get("epsilon", 1e-3)) - BN_EPS) > 1e-12:
            _refuse(n, f"epsilon {c.get('epsilon')} (this backend's BatchNormalization uses {BN_EPS})")
        if not c.get("center", True) or not c.get("scale", True):
            _refuse(n, "center/scale off (gamma and beta are always present here)")
        if c.get("axis", -1) not in (-1, 3, [-1], [3]):
            _refuse(n, f"axis {c.get('axis')!r} (the channel axis expected)")

    def act(self, n: str, kind: str) -> None:
        if self.take(n, "Activation").get("activation") != kind:
            _refuse(n, f"activation {self.cfg(n).get('activation')!r} ({kind!r} expected)")

    def conv_block(self, n: str) -> Tuple[str, str, str, int, float]:
        """Conv2D 3x3 -> BatchNormalization -> relu, starting at conv `n`."""
        f, l2 = self.conv(n, 3, False, "linear")
        b = self.one_user(n)
        self.bn(b)
        a = self.one_user(b)
        self.act(a, "relu")
        return n, b, a, f, l2


def parse_config(config: dict) -> Tuple[Dict[str, Any], Dict[str, Tuple[str, int]]]:
    """config.json of a Keras leaf_cnn -> (build_leafcnn hyperparameters, {weight name:
    (config layer name, variable index)}).  Anything this backend cannot run as the same
    function raises ValueError naming the layer."""
    g = _Graph(config)
    src: Dict[str, Tuple[str, int]] = {}
    ins = [n for n in g.order if g.cls(n) == "InputLayer"]
    if len(ins) != 1:
        _refuse(None, f"{len(ins)} InputLayers (leaf_cnn has one)")
    x = ins[0]
    c = g.take(x, "InputLayer")
    shape = c.get("batch_shape", c.get("batch_input_shape"))
    if not isinstance(shape, list) or len(shape) != 4 or shape[1] != shape[2] or shape[3] != 3 \
            or not isinstance(shape[1], int):
        _refuse(x, f"input shape {shape!r} ([None, S, S, 3] expected)")
    hp: Dict[str, Any] = {"img_size": int(shape[1]), "augment": False, "use_norm": False}

    nxt = g.one_user(x)
    if g.cls(nxt) == "Sequential":
        inner = [L.get("class_name") for L in g.take(nxt, "Sequential").get("layers", [])
                 if L.get("class_name") != "InputLayer"]
        if inner != ["RandomFlip", "RandomRotation", "RandomContrast"]:
            _refuse(nxt, f"Sequential of {inner} (leaf_cnn's augmentation is RandomFlip, "
                         "RandomRotation, RandomContrast)")
        hp["augment"] = True
        x, nxt = nxt, g.one_user(nxt)
    if g.cls(nxt) == "Normalization":
        nc = g.take(nxt, "Normalization")
        if nc.get("axis", -1) not in (-1, 3, [-1], [3]) or nc.get("invert", False) \
                or nc.get("mean") is not None or nc.get("variance") is not None:
            _refuse(nxt, "only an adapted per-channel Normalization(axis=-1) is supported")
        hp["use_norm"] = True
        src["input_norm.mean"], src["input_norm.variance"] = (nxt, 0), (nxt, 1)
        x, nxt = nxt, g.one_user(nxt)

    conv, bn, x, cin, l2 = g.conv_block(nxt)
    src["stem.w"] = (conv, 0)
    _bn_src(src, "stem.bn", bn)
    l2s, widths, se_flags, drops = [l2], [], [], []
    while True:
        users = g.users.get(x, [])
        if len(users) == 1 and g.cls(users[0]) == "GlobalAveragePooling2D":
            break
        i, p = len(widths), f"s{len(widths)}."
        c3 = [u for u in users if g.cls(u) == "Conv2D" and
              _pair(g.cfg(u).get("kernel_size"), "kernel_size", u) == (3, 3)]
        if len(users) != 2 or len(c3) != 1:
            _refuse(x, f"feeds {users}: a residual block (3x3 Conv2D + shortcut) or the head expected")
        c1, b1, a1, f, l2a = g.conv_block(c3[0])
        c2, b2, y, f2, l2b = g.conv_block(g.one_user(a1))
        if f2 != f:
            _refuse(c2, f"{f2} filters after a {f}-filter conv (leaf_cnn's block keeps its width)")
        l2s += [l2a, l2b]
        src[p + "c1.w"], src[p + "c2.w"] = (c1, 0), (c2, 0)
        _bn_src(src, p + "bn1", b1)
        _bn_src(src, p + "bn2", b2)
        yu = g.users.get(y, [])
        gap = [u for u in yu if g.cls(u) == "GlobalAveragePooling2D"]
        if gap:
            if len(yu) != 2 or not g.take(gap[0], "GlobalAveragePooling2D").get("keepdims"):
                _refuse(gap[0], "squeeze-and-excitation pooling must keep dims and share its input "
                                "with the Multiply only")
            s1 = g.one_user(gap[0])
            r, _ = g.conv(s1, 1, True, "relu")
            s2 = g.one_user(s1)
            r2, _ = g.conv(s2, 1, True, "sigmoid")
            if r != f // SE_RATIO or r2 != f:
                _refuse(s1, f"squeeze-and-excitation {f}->{r}->{r2} (ratio {SE_RATIO} expected: "
                            f"{f}->{f // SE_RATIO}->{f})")
            mul = g.one_user(s2)
            g.take(mul, "Multiply")
            if sorted(g.inputs[mul]) != sorted([y, s2]):
                _refuse(mul, f"multiplies {g.inputs[mul]} (the block output and its SE gate expected)")
            src[p + "se.w1"], src[p + "se.b1"] = (s1, 0), (s1, 1)
            src[p + "se.w2"], src[p + "se.b2"] = (s2, 0), (s2, 1)
            y = mul
        se_flags.append(bool(gap))
        add = g.one_user(y)
        g.take(add, "Add")
        short = [s for s in g.inputs[add] if s != y]
        if len(g.inputs[add]) != 2 or len(short) != 1:
            _refuse(add, f"adds {g.inputs[add]} (the block output and its shortcut expected)")
        s = short[0]
        if s != x:
            g.bn(s)
            pc = g.inputs[s][0] if len(g.inputs[s]) == 1 else None
            if pc is None or g.inputs.get(pc) != [x]:
                _refuse(s, "shortcut is neither the block input nor BN(Conv2D 1x1(block input))")
            pf, _ = g.conv(pc, 1, False, "linear")
            if pf != f:
                _refuse(pc, f"projection to {pf} channels in a {f}-wide block")
            src[p + "proj.w"] = (pc, 0)
            _bn_src(src, p + "bnp", s)
        if (s != x) != (cin != f):
            _refuse(add, f"a {cin}->{f} block {'with' if s != x else 'without'} a projection shortcut "
                         "(leaf_cnn projects exactly when the width changes)")
        a = g.one_user(add)
        g.act(a, "relu")
        nxt = g.one_user(a)
        rate = 0.0
        if g.cls(nxt) == "SpatialDropout2D":
            rate = float(g.take(nxt, "SpatialDropout2D").get("rate", 0.0))
            nxt = g.one_user(nxt)
        drops.append(rate)
        pc = g.take(nxt, "MaxPooling2D", "MaxPool2D")
        if _pair(pc.get("pool_size"), "pool_size", nxt) != (2, 2) or \
                _pair(pc.get("strides") or 2, "strides", nxt) != (2, 2) or pc.get("padding", "valid") != "valid":
            _refuse(nxt, "max pooling other than 2x2 / stride 2 / valid")
        widths.append(f)
        x, cin = nxt, f
    if not widths:
        _refuse(x, "no residual block before the head")
    if len(set(se_flags)) != 1 or len(set(drops)) != 1 or len(set(l2s)) != 1:
        _refuse(None, f"blocks differ in squeeze-and-excitation {se_flags}, spatial dropout {drops} or "
                      f"L2 {sorted(set(l2s))} (build_leafcnn uses one setting for all)")
    gap = g.one_user(x)
    if g.take(gap, "GlobalAveragePooling2D").get("keepdims"):
        _refuse(gap, "head pooling keeps dims (leaf_cnn flattens here)")
    nxt = g.one_user(gap)
    drop_top = 0.0
    if g.cls(nxt) == "Dropout":
        drop_top = float(g.take(nxt, "Dropout").get("rate", 0.0))
        nxt = g.one_user(nxt)
    dc = g.take(nxt, "Dense")
    if dc.get("activation") != "softmax" or not dc.get("use_bias", True) or g.users.get(nxt):
        _refuse(nxt, "the head must end in Dense(num_classes, activation='softmax') with a bias")
    src["dense.w"], src["dense.b"] = (nxt, 0), (nxt, 1)
    rest = [n for n in g.order if n not in g.seen]
    if rest:
        _refuse(rest[0], f"{g.cls(rest[0])} is not part of leaf_cnn's graph")
    hp.update(num_classes=int(dc["units"]), widths=widths, use_se=se_flags[0], drop_block=drops[0],
              drop_top=drop_top, l2_reg=l2s[0])
    return hp, src


def _bn_src(src: Dict[str, Tuple[str, int]], base: str, layer: str) -> None:
    for i, v in enumerate(("gamma", "beta", "moving_mean", "moving_variance")):
        src[f"{base}.{v}"] = (layer, i)


def weight_paths(layers: List[dict]) -> Dict[str, str]:
    """{config layer name: its weights group}: saving_lib names each layer of a container by its
    snake_case class name, with a per-class counter, in the container's layer order."""
    used: Dict[str, int] = {}
    out = {}
    for L in layers:
        base = snake_case(L.get("class_name", ""))
        if base in used:
            used[base] += 1
            base = f"{base}_{used[base]}"
        else:
            used[base] = 0
        out[L.get("name") or L.get("config", {}).get("name")] = "layers/" + base
    return out


def weights_from_h5(config: dict, h5: Dict[str, np.ndarray]) -> Tuple[Dict[str, Any], List[str], List[np.ndarray]]:
    """(hyperparameters, weight names, float32 arrays in get_weights() order)."""
    hp, src = parse_config(config)
    paths = weight_paths(config["config"]["layers"])
    counts: Dict[str, int] = defaultdict(int)
    for key in h5:
        m = re.fullmatch(r"(layers/[^/]+)/vars/(\d+)", key)
        if m:
            counts[m.group(1)] = max(counts[m.group(1)], int(m.group(2)) + 1)
    names, arrays = [], []
    expect = {"BatchNormalization": (4,), "Dense": (2,), "Normalization": (2, 3)}
    for name, shape in keras_shapes(hp):
        layer, idx = src[name]
        path = paths[layer]
        cls = next(L["class_name"] for L in config["config"]["layers"]
                   if (L.get("name") or L["config"]["name"]) == layer)
        ok = ((2,) if name.startswith("s") and ".se." in name else (1,)) if cls == "Conv2D" else expect[cls]
        if counts[path] not in ok:
            raise ValueError(f"keras weights: layer {layer!r} ({cls}, {path}) holds {counts[path]} "
                             f"variables ({' or '.join(map(str, ok))} expected)")
        key = f"{path}/vars/{idx}"
        arr = h5[key]
        if arr.dtype.kind != "f":
            raise ValueError(f"keras weights: {key} (layer {layer!r}, {name}) is {arr.dtype}, not float")
        if tuple(arr.shape) != shape:
            raise ValueError(f"keras weights: {key} (layer {layer!r}, {name}) has shape "
                             f"{tuple(arr.shape)}, expected {shape}")
        names.append(name)
        arrays.append(arr.astype(np.float32))
    return hp, names, arrays


def read_archive(path) -> Tuple[Dict[str, Any], List[str], List[np.ndarray]]:
    """A Keras-written leaf_cnn `.keras` zip -> (hyperparameters, weight names, arrays)."""
    with zipfile.ZipFile(path) as z:
        members = set(z.namelist())
        for need in ("config.json", "model.weights.h5"):
            if need not in members:
                raise ValueError(f"{path}: Keras archive without {need}")
        config = json.loads(z.read("config.json"))
        h5 = hdf5.read(z.read("model.weights.h5"))
    try:
        return weights_from_h5(config, h5)
    except KeyError as e:
        raise ValueError(f"{path}: model.weights.h5 lacks {e}") from None


# ===================================================================== writing
def _init(cls: str) -> dict:
    return {"module": "keras.initializers", "class_name": cls, "config": {"seed": None} if cls == "GlorotUniform" else {},
            "registered_name": None}


class _Builder:
    """Records layers the way a fresh Keras session names them (per-class counters in creation
    order) with the shapes of their outputs."""

    def __init__(self, dtype) -> None:
        self.uid: Dict[str, int] = defaultdict(int)
        self.layers: List[dict] = []
        self.shape: Dict[str, list] = {}
        self.dtype = dtype

    def name(self, cls: str) -> str:
        base = snake_case(cls)
        n = self.uid[base]
        self.uid[base] += 1
        return base if n == 0 else f"{base}_{n}"

    def _tensor(self, n: str) -> dict:
        return {"class_name": "__keras_tensor__",
                "config": {"shape": self.shape[n], "dtype": "float32", "keras_history": [n, 0, 0]}}

    def add(self, cls: str, cfg: dict, inputs: List[str], out_shape: list, name: Optional[str] = None,
            module: str = "keras.layers") -> str:
        name = name or self.name(cls)
        in_shapes = [self.shape[i] for i in inputs]
        args = [self._tensor(i) for i in inputs]
        layer = {"module": module, "class_name": cls,
                 "config": {"name": name, "trainable": True, "dtype": self.dtype, **cfg},
                 "registered_name": None, "name": name,
                 "inbound_nodes": [{"args": [args] if len(args) > 1 else args, "kwargs": {}}] if inputs else []}
        if inputs:
            layer["build_config"] = {"input_shape": in_shapes if len(in_shapes) > 1 else in_shapes[0]}
        self.layers.append(layer)
        self.shape[name] = out_shape
        return name

    def conv(self, x: str, f: int, k: int, bias: bool, act: str, l2: float) -> str:
        s = self.shape[x]
        reg = {"module": "keras.regularizers", "class_name": "L2", "config": {"l2": l2},
               "registered_name": None} if l2 > 0 else None
        cfg = {"filters": f, "kernel_size": [k, k], "strides": [1, 1], "padding": "same",
               "data_format": "channels_last", "dilation_rate": [1, 1], "groups": 1, "activation": act,
               "use_bias": bias, "kernel_initializer": _init("GlorotUniform"), "bias_initializer": _init("Zeros"),
               "kernel_regularizer": reg, "bias_regularizer": None, "activity_regularizer": None,
               "kernel_constraint": None, "bias_constraint": None}
        return self.add("Conv2D", cfg, [x], s[:3] + [f])

    def bn(self, x: str) -> str:
        cfg = {"axis": -1, "momentum": 0.99, "epsilon": BN_EPS, "center": True, "scale": True,
               "beta_initializer": _init("Zeros"), "gamma_initializer": _init("Ones"),
               "moving_mean_initializer": _init("Zeros"), "moving_variance_initializer": _init("Ones"),
               "beta_regularizer": None, "gamma_regularizer": None, "beta_constraint": None,
               "gamma_constraint": None}
        return self.add("BatchNormalization", cfg, [x], self.shape[x])

    def act(self, x: str, kind: str) -> str:
        return self.add("Activation", {"activation": kind}, [x], self.shape[x])

    def conv_block(self, x: str, f: int, l2: float) -> str:
        return self.act(self.bn(self.conv(x, f, 3, False, "linear", l2)), "relu")


def functional_config(hp: Dict[str, Any], dtype="float32") -> dict:
    """The Keras 3 config.json of the reference's build_leafcnn(**hp) in a fresh session."""
    b = _Builder(dtype)
    s = int(hp["img_size"])
    shape = [None, s, s, 3]
    x = b.name("InputLayer")
    b.layers.append({"module": "keras.layers", "class_name": "InputLayer",
                     "config": {"batch_shape": shape, "dtype": "float32", "sparse": False, "name": x},
                     "registered_name": None, "name": x, "inbound_nodes": []})
    b.shape[x] = shape
    if hp["augment"]:
        inner = [("RandomFlip", {"mode": "horizontal", "seed": None}),
                 ("RandomRotation", {"factor": 0.05, "fill_mode": "reflect", "interpolation": "bilinear",
                                     "seed": None, "fill_value": 0.0}),
                 ("RandomContrast", {"factor": 0.1, "seed": None})]
        inner_cfg = [{"module": "keras.layers", "class_name": c,
                      "config": {"name": b.name(c), "trainable": True, "dtype": dtype, **cfg},
                      "registered_name": None} for c, cfg in inner]
        seq_input = b.name("InputLayer")        # built when the Sequential is first called
        inner_cfg.insert(0, {"module": "keras.layers", "class_name": "InputLayer",
                             "config": {"batch_shape": shape, "dtype": "float32", "sparse": False,
                                        "name": seq_input}, "registered_name": None})
        x = b.add("Sequential", {"layers": inner_cfg, "build_input_shape": shape}, [x], shape,
                  name="augment", module="keras")
    if hp["use_norm"]:
        x = b.add("Normalization", {"axis": [-1], "invert": False, "mean": None, "variance": None},
                  [x], shape, name="input_norm")
    widths, l2 = list(hp["widths"]), float(hp["l2_reg"] or 0.0)
    x = b.conv_block(x, widths[0], l2)
    for f in widths:
        short = x
        y = b.conv_block(b.conv_block(x, f, l2), f, l2)
        if hp["use_se"]:
            h, w = b.shape[y][1:3]
            g = b.add("GlobalAveragePooling2D", {"data_format": "channels_last", "keepdims": True}, [y],
                      [None, 1, 1, f])
            g = b.conv(g, f // SE_RATIO, 1, True, "relu", 0.0)
            g = b.conv(g, f, 1, True, "sigmoid", 0.0)
            y = b.add("Multiply", {}, [y, g], b.shape[y])
        if b.shape[short][3] != f:
            short = b.bn(b.conv(short, f, 1, False, "linear", 0.0))
        y = b.add("Add", {}, [short, y], b.shape[y])
        x = b.act(y, "relu")
        if hp["drop_block"] and hp["drop_block"] > 0:
            x = b.add("SpatialDropout2D", {"rate": float(hp["drop_block"]), "seed": None,
                                           "data_format": "channels_last"}, [x], b.shape[x])
        sh = b.shape[x]
        x = b.add("MaxPooling2D", {"pool_size": [2, 2], "padding": "valid", "strides": [2, 2],
                                   "data_format": "channels_last"}, [x], [None, sh[1] // 2, sh[2] // 2, sh[3]])
    x = b.add("GlobalAveragePooling2D", {"data_format": "channels_last", "keepdims": False}, [x],
              [None, widths[-1]])
    if hp["drop_top"] and hp["drop_top"] > 0:
        x = b.add("Dropout", {"rate": float(hp["drop_top"]), "seed": None, "noise_shape": None}, [x], b.shape[x])
    n = int(hp["num_classes"])
    out = b.add("Dense", {"units": n, "activation": "softmax", "use_bias": True,
                          "kernel_initializer": _init("GlorotUniform"), "bias_initializer": _init("Zeros"),
                          "kernel_regularizer": None, "bias_regularizer": None, "kernel_constraint": None,
                          "bias_constraint": None}, [x], [None, n])
    layers = _graph_order(b.layers, out)
    return {"module": "keras.src.models.functional", "class_name": "Functional",
            "config": {"name": "leaf_cnn", "trainable": True, "layers": layers,
                       "input_layers": [layers[0]["name"], 0, 0], "output_layers": [out, 0, 0]},
            "registered_name": "Functional", "build_config": {"input_shape": None}}


def _graph_order(layers: List[dict], output: str) -> List[dict]:
    """Functional.layers order (keras.src.ops.function.map_graph): layers by decreasing depth
    (longest path to the output), ties by first visit of a depth-first walk from the output
    that follows each layer's inputs in order."""
    by = {L["name"]: L for L in layers}
    ins = {n: _inbound(L, n) for n, L in by.items()}
    index: Dict[str, int] = {}
    post: List[str] = []

    def visit(n: str) -> None:
        if n in post:
            return
        index.setdefault(n, len(index))
        for i in ins[n]:
            visit(i)
        post.append(n)

    visit(output)
    depth: Dict[str, int] = {}
    for n in reversed(post):             # consumers before producers
        d = depth.setdefault(n, 0)
        for i in ins[n]:
            depth[i] = max(depth.get(i, 0), d + 1)
    return [by[n] for n in sorted(post, key=lambda n: (-depth[n], index[n]))]


def _seed_state() -> np.ndarray:
    return np.zeros(2, np.int64)


def weights_tree(config: dict, hp: Dict[str, Any], names: List[str], arrays: List[np.ndarray]) -> dict:
    """The model.weights.h5 tree Keras 3's loader walks for `config`'s layers."""
    _hp, src = parse_config(config)
    paths = weight_paths(config["config"]["layers"])
    vals = dict(zip(names, arrays))
    tree: dict = {"layers": {}, "vars": {}}
    groups: Dict[str, dict] = {}
    for L in config["config"]["layers"]:
        group = {"vars": {}}
        cls = L["class_name"]
        if cls == "Normalization":
            group["vars"]["2"] = np.array(0, np.int64)          # adapt()'s sample count: unused once adapted
        if cls in ("SpatialDropout2D", "Dropout"):
            group["seed_generator"] = {"vars": {"0": _seed_state()}}
        if cls == "Sequential":
            inner = {}
            for c in ("random_flip", "random_rotation", "random_contrast"):
                inner[c] = {"vars": {}, "generator": {"vars": {"0": _seed_state()}}}
            group["layers"] = inner
        tree["layers"][paths[L["name"]][len("layers/"):]] = group
        groups[L["name"]] = group
    for name, (layer, idx) in src.items():
        groups[layer]["vars"][str(idx)] = np.asarray(vals[name], np.float32)
    return tree


def write_archive(path, hp: Dict[str, Any], names: List[str], arrays: List[np.ndarray]) -> None:
    """A Keras 3 `.keras` zip for the leaf_cnn `hp` describes, holding `arrays` (get_weights() order)."""
    expect = keras_shapes(hp)
    if [n for n, _s in expect] != list(names):
        raise ValueError("write_archive: weight names do not match the model's hyperparameters")
    for (n, s), a in zip(expect, arrays):
        if tuple(np.shape(a)) != s:
            raise ValueError(f"write_archive: {n} has shape {np.shape(a)}, expected {s}")
    config = functional_config(hp)
    h5 = hdf5.write(None, weights_tree(config, hp, names, arrays))
    meta = {"keras_version": KERAS_VERSION,
            "date_saved": datetime.datetime.now().strftime("%Y-%m-%d@%H:%M:%S")}
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        z.writestr("metadata.json", json.dumps(meta))
        z.writestr("config.json", json.dumps(config))
        z.writestr("model.weights.h5", h5)


def is_keras_archive(path) -> bool:
    try:
        with zipfile.ZipFile(path) as z:
            return "model.weights.h5" in z.namelist()
    except (zipfile.BadZipFile, OSError):
        return False


__all__ = ["parse_config", "functional_config", "read_archive", "write_archive", "weights_from_h5",
           "weights_tree", "weight_paths", "keras_shapes", "snake_case", "is_keras_archive", "KERAS_VERSION"]
