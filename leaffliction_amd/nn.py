"""Host-side launchers for the leaf_cnn kernels of libleafhip.so (fp32, NCHW)."""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from . import _lib
from .ops import _chk, _stream

_F32 = torch.float32
_BF16 = torch.bfloat16
_ws_cache = {}
_ws_gen = 0
# A/B knob for measurements: route BatchNorm backward through the standalone apply kernel
_NO_FUSED_BN_WGRAD = os.environ.get("LEAFFLICTION_NO_FUSED_BN_WGRAD", "0") == "1"
# A/B knob for measurements: the projection shortcut's backward as bn_bwd_wgrad + the 1x1 input-gradient convolution
_NO_FUSED_PROJ_BWD = os.environ.get("LEAFFLICTION_NO_FUSED_PROJ_BWD", "0") == "1"
# A/B knob for measurements: the fp32 tail backward gathers y / sc_y from the full-size planes (no y_at / sc_at)
_NO_TAIL_KEEP = os.environ.get("LEAFFLICTION_NO_TAIL_KEEP", "0") == "1"


def _workspace(nbytes: int, device, slot: int = 0) -> torch.Tensor:
    """Grow-only scratch buffer per device and slot (the C ABI never allocates).

    A buffer that is replaced goes back to torch's allocator, so every pointer taken from it is dead from then on.
    `workspace_generation()` counts the replacements: whoever keeps such pointers beyond the call — the HIP graph of
    the training step has them baked into its kernel nodes — compares generations and re-records (model/cnn.py)."""
    global _ws_gen
    key = (str(device), slot)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a workspace would have to grow while a HIP graph is being recorded: run the shape "
                               "eagerly first (the warm-up steps size every workspace)")
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
        _ws_gen += 1
    return buf


def workspace_generation() -> int:
    """Number of times a workspace buffer has been (re)allocated in this process; see _workspace."""
    return _ws_gen


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def conv2d_takes_wino_filters(cin: int, h: int, w: int, cout: int, ksize: int) -> bool:
    """Whether conv2d / conv2d_bn_stats / conv2d_bnbwd run this shape in the Winograd domain (every 3x3 but the
    Cin <= 4 stem) and so read conv2d_wino_filters' output instead of the raw weights."""
    return bool(_lib.load().lf_conv2d_takes_wino_filters(int(cin), int(h), int(w), int(cout), int(ksize)))


def conv2d_wino_filters(w_iko: torch.Tensor, dgrad: bool = False,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3 weights [Cin,9,Cout] -> their Winograd F(2x2,3x3) transforms U = G g G^T, the `wino_u` of conv2d /
    conv2d_bn_stats / conv2d_bnbwd: [Cin,Cout,16] for the forward convolution, or with `dgrad` [Cout,Cin,16] from
    the flipped taps for the input-gradient convolution (no conv2d_dgrad_weights in between).  The weights change
    once per optimizer step: prepare once per layer, role and step."""
    _chk(w_iko, _F32, "conv2d_wino_filters.w", 3)
    cin, taps, cout = w_iko.shape
    if taps != 9:
        raise ValueError("conv2d_wino_filters: 3x3 weights [Cin,9,Cout] expected")
    shape = (cout, cin, 16) if dgrad else (cin, cout, 16)
    if out is None:
        out = torch.empty(shape, dtype=_F32, device=w_iko.device)
    else:
        _chk(out, _F32, "conv2d_wino_filters.out", 3)
        if tuple(out.shape) != shape:
            raise ValueError(f"conv2d_wino_filters.out: expected {shape}")
    _lib.call("lf_conv2d_wino_filters_f32", w_iko.data_ptr(), out.data_ptr(), cin, cout, 1 if dgrad else 0,
              _stream())
    return out


def _conv_weights(who: str, x: torch.Tensor, w_iko: Optional[torch.Tensor], ksize: int,
                  wino_u: Optional[torch.Tensor]):
    """Checks the weights of a convolution launch; returns (cout, w pointer, wino_u pointer).  A launch that runs
    in the Winograd domain reads U: the caller's prepared `wino_u` (w_iko may then be None), or else U prepared
    here from w_iko into a workspace slot, one tiny launch.  Every other launch reads w_iko."""
    n, cin, h, w = x.shape
    if w_iko is not None:
        _chk(w_iko, _F32, f"{who}.w", 3)
        if w_iko.shape[0] != cin or w_iko.shape[1] != ksize * ksize:
            raise ValueError(f"{who}.w: expected [{cin},{ksize * ksize},Cout], got {tuple(w_iko.shape)}")
        cout = w_iko.shape[2]
    elif wino_u is not None:
        cout = wino_u.shape[1] if wino_u.dim() == 3 else 0
    else:
        raise ValueError(f"{who}: no weights")
    if not conv2d_takes_wino_filters(cin, h, w, cout, ksize):
        if w_iko is None:
            raise ValueError(f"{who}: this launch reads the raw weights, not wino_u")
        return cout, w_iko.data_ptr(), None
    if wino_u is None:
        ws = _workspace(cin * cout * 64, x.device, slot=3)
        wino_u = conv2d_wino_filters(w_iko, out=ws[:cin * cout * 64].view(_F32).view(cin, cout, 16))
    else:
        _chk(wino_u, _F32, f"{who}.wino_u", 3)
        if tuple(wino_u.shape) != (cin, cout, 16):
            raise ValueError(f"{who}.wino_u: expected [{cin},{cout},16], got {tuple(wino_u.shape)}")
    return cout, _ptr(w_iko), wino_u.data_ptr()


# The rules every convolution launcher below shares, each stated once.
def _prologue(who: str, in_scale, in_shift, cin: int) -> None:
    """The prologue x' = x*in_scale[c]+in_shift[c] of a launch: f32 vectors [Cin], or None."""
    for t, nm in ((in_scale, "in_scale"), (in_shift, "in_shift")):
        if t is not None:
            _chk(t, _F32, f"{who}.{nm}", 1)
            if t.shape[0] != cin:
                raise ValueError(f"{who}.{nm}: expected [{cin}]")


def _act_in(who: str, x: torch.Tensor) -> bool:
    """Checks an input stored as fp32 or bf16 (contiguous NCHW); True for bf16."""
    if x.dtype not in (_F32, _BF16):
        raise TypeError(f"{who}.x: expected float32 or bfloat16, got {x.dtype}")
    _chk(x, x.dtype, f"{who}.x", 4)
    return x.dtype == _BF16


def _act_out(who: str, out: Optional[torch.Tensor], shape, dtypes, default, device) -> torch.Tensor:
    """The output of a launch: `out`, or a new tensor of dtype `default` (None: `out` is required); either way
    contiguous, of one of `dtypes` and of `shape`."""
    if out is None and default is not None:
        out = torch.empty(shape, dtype=default, device=device)
    dtype = getattr(out, "dtype", None)
    _chk(out, dtype if dtype in dtypes else dtypes[0], f"{who}.out", len(shape))
    if tuple(out.shape) != shape:
        raise ValueError(f"{who}.out: expected {shape}, got {tuple(out.shape)}")
    return out


def _bf16_weight_elems(cin: int, cout: int, ksize: int) -> int:
    """lf_conv2d_bf16_weight_elems in Python, for the launchers' checks (no library call per launch)."""
    return ((cin + 15) // 16) * ksize * ksize * cout * 16


def _packed_weights(who: str, wprep: torch.Tensor, cin: int, cout: int, ksize: int) -> None:
    if wprep.dtype != torch.int16 or wprep.numel() != _bf16_weight_elems(cin, cout, ksize):
        raise ValueError(f"{who}.wprep: not the packed weights of this convolution")


def _tile_part(x: torch.Tensor, tiles: int, cout: int) -> torch.Tensor:
    """Workspace (slot 1) for the per-tile sums [tiles,Cout,2] a convolution's statistics epilogue leaves."""
    return _workspace(tiles * cout * 8, x.device, slot=1)


def _bn_stats_from_tiles(tp, tiles, n, cout, hw, gamma, beta, mmean, mvar, stats, momentum, eps, device) -> None:
    """BatchNorm training statistics `stats` [4,C] and the moving statistics from a convolution's per-tile sums."""
    ws = _workspace(_lib.load().lf_bn_workspace(cout), device)
    _lib.call("lf_bn_train_stats_tiles_f32", tp.data_ptr(), tiles, n, cout, hw, gamma.data_ptr(), beta.data_ptr(),
              mmean.data_ptr(), mvar.data_ptr(), float(momentum), float(eps), stats[0].data_ptr(),
              stats[1].data_ptr(), stats[2].data_ptr(), stats[3].data_ptr(), ws.data_ptr(), ws.numel(), _stream())


def _bn_bwd_coef(who: str, stats, gamma, dgamma, dbeta, relu: bool, n: int, c: int, hw: int, device, g=None,
                 y=None, alpha_nc=None, add_nc=None, plane_g=None, plane_m=None, tile_sums=None):
    """The reduction half of BatchNorm backward: fills dgamma / dbeta and the per-channel coefficients `coef`
    (slot 2) from which a kernel forms dy = BN'(g).  Exactly one source of sums: tile_sums (a convolution's
    epilogue: final, so no alpha/add/plane sums next to them), plane_g (+ plane_m), or a pass over g and y.
    Returns (coef, the BatchNorm workspace)."""
    beside = any(t is not None for t in (alpha_nc, add_nc, plane_g))
    if (beside if tile_sums is not None else (plane_g is None and g is None)):
        raise ValueError(f"{who}: sums from tile_sums alone (no alpha/add/plane sums), or else from plane_g or g, y")
    coef = _workspace(5 * c * 4, device, slot=2)
    ws = _workspace(_lib.load().lf_bn_workspace(c), device)
    if tile_sums is not None:
        tp, tiles = tile_sums
        _lib.call("lf_bn_bwd_sums_tiles_f32", tp.data_ptr(), tiles, stats[0].data_ptr(), stats[1].data_ptr(),
                  stats[2].data_ptr(), stats[3].data_ptr(), gamma.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                  coef.data_ptr(), n, c, hw, ws.data_ptr(), ws.numel(), _stream())
    else:
        _lib.call("lf_bn_bwd_sums_f32", _ptr(g), _ptr(alpha_nc), _ptr(add_nc), _ptr(y), stats[0].data_ptr(),
                  stats[1].data_ptr(), stats[2].data_ptr(), stats[3].data_ptr(), 1 if relu else 0, gamma.data_ptr(),
                  dgamma.data_ptr(), dbeta.data_ptr(), coef.data_ptr(), _ptr(plane_g), _ptr(plane_m), n, c, hw,
                  ws.data_ptr(), ws.numel(), _stream())
    return coef, ws


def conv2d(x: torch.Tensor, w_iko: Optional[torch.Tensor], ksize: int, in_scale=None, in_shift=None,
           in_relu: bool = False, out: Optional[torch.Tensor] = None,
           accumulate: bool = False, wino_u: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = conv2d_same(x', w); x' = relu?(x*in_scale[c]+in_shift[c]) if a prologue is given.

    x [N,Cin,H,W] f32, w_iko [Cin, k*k, Cout] f32 -> y [N,Cout,H,W].  wino_u: conv2d_wino_filters' output for a
    3x3 convolution (see _conv_weights).
    """
    _chk(x, _F32, "conv2d.x", 4)
    n, cin, h, w = x.shape
    cout, w_ptr, u_ptr = _conv_weights("conv2d", x, w_iko, ksize, wino_u)
    _prologue("conv2d", in_scale, in_shift, cin)
    if out is None and accumulate:
        raise ValueError("conv2d: accumulate needs an output tensor")
    out = _act_out("conv2d", out, (n, cout, h, w), (_F32,), _F32, x.device)
    _lib.call("lf_conv2d_f32", x.data_ptr(), w_ptr, out.data_ptr(), n, cin, h, w, cout,
              ksize, _ptr(in_scale), _ptr(in_shift), 1 if in_relu else 0, 1 if accumulate else 0,
              _stream(), u_ptr)
    return out


def conv2d_bf16_weights(w_iko: torch.Tensor, ksize: int) -> torch.Tensor:
    """Pack fp32 IKO weights [Cin, k*k, Cout] for conv2d_bf16 (uint16 view of bf16
    [ceil(Cin/16), k*k, Cout, 16])."""
    _chk(w_iko, _F32, "conv2d_bf16_weights.w", 3)
    cin, taps, cout = w_iko.shape
    if taps != ksize * ksize:
        raise ValueError(f"conv2d_bf16_weights.w: expected [{cin},{ksize * ksize},Cout]")
    n = int(_lib.load().lf_conv2d_bf16_weight_elems(cin, cout, ksize))
    out = torch.empty(n, dtype=torch.int16, device=w_iko.device)
    _lib.call("lf_conv2d_bf16_prep_weights", w_iko.data_ptr(), out.data_ptr(), cin, cout, ksize, _stream())
    return out


def conv2d_bf16(x: torch.Tensor, wprep: torch.Tensor, cout: int, ksize: int, in_scale=None, in_shift=None,
                in_relu: bool = False, out: Optional[torch.Tensor] = None,
                out_dtype: torch.dtype = torch.float32, out_scale=None, out_shift=None,
                out_relu: bool = False) -> torch.Tensor:
    """conv2d with bf16 operands / fp32 accumulation (inference).  x: fp32 or bf16 NCHW; the result
    is fp32 or bf16 NCHW (`out_dtype`, or the dtype of `out`); wprep from conv2d_bf16_weights.
    out_scale / out_shift [Cout] (+ out_relu): epilogue on the accumulators (folded BatchNorm)."""
    xb = _act_in("conv2d_bf16", x)
    n, cin, h, w = x.shape
    _packed_weights("conv2d_bf16", wprep, cin, cout, ksize)
    _prologue("conv2d_bf16", in_scale, in_shift, cin)
    out = _act_out("conv2d_bf16", out, (n, cout, h, w), (_F32, _BF16), out_dtype, x.device)
    _lib.call("lf_conv2d_bf16_act", x.data_ptr(), 1 if xb else 0, wprep.data_ptr(),
              out.data_ptr(), 1 if out.dtype == _BF16 else 0, n, cin, h, w, cout, ksize,
              _ptr(in_scale), _ptr(in_shift), 1 if in_relu else 0, _ptr(out_scale), _ptr(out_shift),
              1 if out_relu else 0, _stream())
    return out


def conv2d_bf16_mean(x: torch.Tensor, wprep: torch.Tensor, cout: int, ksize: int, out: torch.Tensor,
                     means: torch.Tensor, in_scale=None, in_shift=None, in_relu: bool = False, out_scale=None,
                     out_shift=None, out_relu: bool = False):
    """conv2d_bf16 with bf16 output AND the per-image channel means of the stored activation, taken in the
    convolution's epilogue (inference: a block's second convolution + the squeeze of its SE gate in one pass).
    x: fp32 or bf16 NCHW; out: bf16 [N,Cout,H,W]; means: fp32 [N,Cout].  Returns (out, means)."""
    xb = 1 if _act_in("conv2d_bf16_mean", x) else 0
    n, cin, h, w = x.shape
    _packed_weights("conv2d_bf16_mean", wprep, cin, cout, ksize)
    _prologue("conv2d_bf16_mean", in_scale, in_shift, cin)
    _act_out("conv2d_bf16_mean", out, (n, cout, h, w), (_BF16,), None, x.device)
    _chk(means, _F32, "conv2d_bf16_mean.means", 2)
    if tuple(means.shape) != (n, cout):
        raise ValueError("conv2d_bf16_mean.means: expected [N,Cout]")
    ws = _workspace(int(_lib.load().lf_conv2d_bf16_act_mean_workspace(n, cin, h, w, cout, ksize, xb)), x.device, slot=1)
    _lib.call("lf_conv2d_bf16_act_mean", x.data_ptr(), xb, wprep.data_ptr(), out.data_ptr(), n, cin, h, w, cout, ksize,
              _ptr(in_scale), _ptr(in_shift), 1 if in_relu else 0, _ptr(out_scale), _ptr(out_shift),
              1 if out_relu else 0, means.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return out, means


# ---------------------------------------------------------------------------
# mixed-precision training step: bf16 storage, fp32 arithmetic (lf_*_bf16 / *_train_bf16)
# ---------------------------------------------------------------------------
def conv2d_bf16_dgrad_weights(w_iko: torch.Tensor, ksize: int) -> torch.Tensor:
    """Packed bf16 weights of the input-gradient convolution of a conv with fp32 IKO weights w."""
    return conv2d_bf16_weights(conv2d_dgrad_weights(w_iko, ksize), ksize)


def conv2d_bf16_train(x: torch.Tensor, wprep: torch.Tensor, cout: int, ksize: int, out: torch.Tensor,
                      in_scale=None, in_shift=None, in_relu: bool = False, accumulate: bool = False,
                      stats: bool = False, pivot=None, mask_y=None, mask_scale=None, mask_shift=None,
                      mask_relu: bool = False):
    """Forward / input-gradient convolution of the bf16 training step: out (bf16 NCHW) = conv(x')
    (+ out when accumulate).  With stats=True returns (out, (tile_part, tiles)) — BatchNorm forward
    statistics about `pivot`, or (mask_y given) the backward sums of the BatchNorm out feeds."""
    xb = 1 if _act_in("conv2d_bf16_train", x) else 0
    n, cin, h, w = x.shape
    _packed_weights("conv2d_bf16_train", wprep, cin, cout, ksize)
    _act_out("conv2d_bf16_train", out, (n, cout, h, w), (_BF16,), None, x.device)
    _prologue("conv2d_bf16_train", in_scale, in_shift, cin)
    tp, tiles = None, 0
    if mask_y is not None:
        _chk(mask_y, _BF16, "conv2d_bf16_train.mask_y", 4)
        if mask_y.shape != out.shape or mask_scale.shape[0] != cout or mask_shift.shape[0] != cout:
            raise ValueError("conv2d_bf16_train: mask shape mismatch")
        stats = True
    if stats:
        tiles = int(_lib.load().lf_conv2d_bf16_stats_tiles(n, cin, h, w, cout, ksize, xb))
        tp = _tile_part(x, tiles, cout)
    _lib.call("lf_conv2d_bf16_train", x.data_ptr(), xb, wprep.data_ptr(),
              out.data_ptr(), n, cin, h, w, cout, ksize, _ptr(in_scale), _ptr(in_shift),
              1 if in_relu else 0, 1 if accumulate else 0, _ptr(tp), tp.numel() if tp is not None else 0,
              _ptr(pivot), _ptr(mask_y), _ptr(mask_scale), _ptr(mask_shift), 1 if mask_relu else 0,
              _stream())
    return (out, (tp, tiles)) if stats else out


def conv2d_bn_stats_bf16(x, wprep, cout: int, ksize: int, gamma, beta, mmean, mvar, stats: torch.Tensor,
                         in_scale=None, in_shift=None, in_relu: bool = False, out=None,
                         momentum: float = 0.99, eps: float = 1e-3) -> torch.Tensor:
    """Conv2D + training-mode BatchNormalization statistics on bf16 storage: the statistics are
    those of the ROUNDED output (what the next kernels read)."""
    n, _cin, h, w = x.shape
    out, (tp, tiles) = conv2d_bf16_train(x, wprep, cout, ksize, out, in_scale, in_shift, in_relu,
                                         stats=True, pivot=mmean)
    _bn_stats_from_tiles(tp, tiles, n, cout, h * w, gamma, beta, mmean, mvar, stats, momentum, eps, x.device)
    return out


def _bn_bwd_wgrad_checks(who: str, act, x, g, y_bn, dy_out, dw_out, ksize, in_scale, in_shift, alpha_nc, add_nc,
                         plane_g, plane_m):
    """What bn_bwd_wgrad (act f32) and bn_bwd_wgrad_bf16 (act bf16) check next to x: g, y_bn, dy_out [N,Cout,H,W]
    of dtype `act`, dw_out f32 [Cin,k*k,Cout], the prologue, plane sums [N,Cout,2], alpha/add [N,Cout].  Returns
    (n, cin, h, w, cout)."""
    _chk(g, act, f"{who}.g", 4)
    _chk(y_bn, act, f"{who}.y", 4)
    if dy_out is not None:
        _chk(dy_out, act, f"{who}.dy_out", 4)
    _chk(dw_out, _F32, f"{who}.dw_out", 3)
    n, cin, h, w = x.shape
    cout = g.shape[1]
    if g.shape != y_bn.shape or (dy_out is not None and dy_out.shape != g.shape) or g.shape[0] != n \
            or tuple(g.shape[2:]) != (h, w) or tuple(dw_out.shape) != (cin, ksize * ksize, cout):
        raise ValueError(f"{who}: shape mismatch")
    _prologue(who, in_scale, in_shift, cin)
    for t in (plane_g, plane_m):
        if t is not None and tuple(t.shape) != (n, cout, 2):
            raise ValueError(f"{who}: plane sums must be [N,C,2]")
    for t in (alpha_nc, add_nc):
        if t is not None and tuple(t.shape) != (n, cout):
            raise ValueError(f"{who}: alpha/add must be [N,C]")
    return n, cin, h, w, cout


def bn_bwd_wgrad_bf16(x: torch.Tensor, g: torch.Tensor, y_bn: torch.Tensor, stats: torch.Tensor, gamma,
                      dgamma, dbeta, relu: bool, ksize: int, dw_out: torch.Tensor, dy_out,
                      in_scale=None, in_shift=None, in_relu: bool = False, alpha_nc=None, add_nc=None,
                      plane_g=None, plane_m=None, tile_sums=None):
    """bn_bwd_wgrad on bf16 tensors: the BatchNorm-backward sums come from per-plane sums
    (block_tail_bwd / gap) or per-tile sums (conv2d_bf16_train's epilogue) — never
    from another pass over g and y — and dY = BN'(g) is formed inside the weight-gradient kernel."""
    who = "bn_bwd_wgrad_bf16"
    _act_in(who, x)   # float32 for the stem
    n, cin, h, w, cout = _bn_bwd_wgrad_checks(who, _BF16, x, g, y_bn, dy_out, dw_out, ksize, in_scale, in_shift,
                                              alpha_nc, add_nc, plane_g, plane_m)
    coef, _ = _bn_bwd_coef(who, stats, gamma, dgamma, dbeta, relu, n, cout, h * w, x.device, alpha_nc=alpha_nc,
                           add_nc=add_nc, plane_g=plane_g, plane_m=plane_m, tile_sums=tile_sums)
    ws = _workspace(_lib.load().lf_conv2d_wgrad_bf16_workspace(n, cin, h, w, cout, ksize), x.device)
    _lib.call("lf_conv2d_wgrad_bf16", x.data_ptr(), g.data_ptr(), y_bn.data_ptr(), _ptr(alpha_nc),
              _ptr(add_nc), coef.data_ptr(), 1 if relu else 0, _ptr(dy_out), dw_out.data_ptr(), n, cin,
              h, w, cout, ksize, _ptr(in_scale), _ptr(in_shift), 1 if in_relu else 0, ws.data_ptr(),
              ws.numel(), _stream())
    return dy_out


def conv2d_wgrad_bf16(x: torch.Tensor, dy: torch.Tensor, ksize: int, in_scale=None, in_shift=None,
                      in_relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dw [Cin,k*k,Cout] (fp32) = sum x'[n,ci,y+ky-1,x+kx-1] * dy[n,co,y,x] from bf16 tensors."""
    _chk(dy, _BF16, "wgrad_bf16.dy", 4)
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    _prologue("wgrad_bf16", in_scale, in_shift, cin)
    if out is None:
        out = torch.empty((cin, ksize * ksize, cout), dtype=_F32, device=x.device)
    ws = _workspace(_lib.load().lf_conv2d_wgrad_bf16_workspace(n, cin, h, w, cout, ksize), x.device)
    _lib.call("lf_conv2d_wgrad_bf16", x.data_ptr(), dy.data_ptr(), None, None, None, None, 0, None,
              out.data_ptr(), n, cin, h, w, cout, ksize, _ptr(in_scale), _ptr(in_shift),
              1 if in_relu else 0, ws.data_ptr(), ws.numel(), _stream())
    return out


def cast_f32_bf16(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    _lib.call("lf_cast_f32_bf16", src.data_ptr(), dst.data_ptr(), src.numel(), _stream())
    return dst


def cast_bf16_f32(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    _lib.call("lf_cast_bf16_f32", src.data_ptr(), dst.data_ptr(), src.numel(), _stream())
    return dst


def conv2d_bn_stats(x: torch.Tensor, w_iko: Optional[torch.Tensor], ksize: int, gamma, beta, mmean, mvar,
                    stats: torch.Tensor, in_scale=None, in_shift=None, in_relu: bool = False,
                    out: Optional[torch.Tensor] = None, momentum: float = 0.99,
                    eps: float = 1e-3, wino_u: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv2D + training-mode BatchNormalization statistics: y = conv(x'), and `stats` [4,C]
    (mean, invstd, scale, shift) + the moving statistics are produced from per-tile sums the
    convolution gathers in its epilogue, so y is not read again."""
    _chk(x, _F32, "conv2d_bn_stats.x", 4)
    n, cin, h, w = x.shape
    cout, w_ptr, u_ptr = _conv_weights("conv2d_bn_stats", x, w_iko, ksize, wino_u)
    _prologue("conv2d_bn_stats", in_scale, in_shift, cin)
    for t in (gamma, beta, mmean, mvar):
        _chk(t, _F32, "conv2d_bn_stats.param", 1)
        if t.shape[0] != cout:
            raise ValueError("conv2d_bn_stats: per-channel vectors must be [Cout]")
    _chk(stats, _F32, "conv2d_bn_stats.stats", 2)
    if tuple(stats.shape) != (4, cout):
        raise ValueError("conv2d_bn_stats.stats: expected [4,Cout]")
    out = _act_out("conv2d_bn_stats", out, (n, cout, h, w), (_F32,), _F32, x.device)
    tiles = _lib.load().lf_conv2d_stats_tiles(n, cin, h, w, cout, ksize)
    tp = _tile_part(x, tiles, cout)
    _lib.call("lf_conv2d_stats_f32", x.data_ptr(), w_ptr, out.data_ptr(), n, cin, h, w,
              cout, ksize, _ptr(in_scale), _ptr(in_shift), 1 if in_relu else 0, mmean.data_ptr(),
              tp.data_ptr(), tp.numel(), _stream(), u_ptr)
    _bn_stats_from_tiles(tp, tiles, n, cout, h * w, gamma, beta, mmean, mvar, stats, momentum, eps, x.device)
    return out


def conv2d_bnbwd(x: torch.Tensor, w_iko: Optional[torch.Tensor], ksize: int, mask_y: torch.Tensor,
                 stats: torch.Tensor, relu: bool, out: torch.Tensor, accumulate: bool = False,
                 wino_u: Optional[torch.Tensor] = None):
    """Input-gradient convolution out (+)= conv(x, w) whose result feeds the backward of the
    BatchNormalization with input mask_y / statistics `stats`: the epilogue also leaves the
    per-tile sums of that BN backward.  Returns (out, tile_sums) — pass tile_sums to
    bn_bwd_wgrad."""
    _chk(x, _F32, "conv2d_bnbwd.x", 4)
    _chk(mask_y, _F32, "conv2d_bnbwd.mask_y", 4)
    n, cin, h, w = x.shape
    cout, w_ptr, u_ptr = _conv_weights("conv2d_bnbwd", x, w_iko, ksize, wino_u)
    _act_out("conv2d_bnbwd", out, (n, cout, h, w), (_F32,), None, x.device)
    if mask_y.shape != out.shape or tuple(stats.shape) != (4, cout):
        raise ValueError("conv2d_bnbwd: shape mismatch")
    tiles = _lib.load().lf_conv2d_stats_tiles(n, cin, h, w, cout, ksize)
    tp = _tile_part(x, tiles, cout)
    _lib.call("lf_conv2d_bnbwd_f32", x.data_ptr(), w_ptr, out.data_ptr(), n, cin, h, w,
              cout, ksize, 1 if accumulate else 0, mask_y.data_ptr(), stats[2].data_ptr(),
              stats[3].data_ptr(), 1 if relu else 0, tp.data_ptr(), tp.numel(), _stream(), u_ptr)
    return out, (tp, tiles)


def conv2d_dgrad_weights(w_iko: torch.Tensor, ksize: int) -> torch.Tensor:
    """[Cin,k*k,Cout] -> [Cout,k*k(flipped),Cin]: conv2d(dy, wt) is the input gradient."""
    _chk(w_iko, _F32, "dgrad_weights.w", 3)
    cin, taps, cout = w_iko.shape
    if taps != ksize * ksize:
        raise ValueError("dgrad_weights: taps != ksize^2")
    wt = torch.empty((cout, taps, cin), dtype=_F32, device=w_iko.device)
    _lib.call("lf_conv2d_dgrad_weights_f32", w_iko.data_ptr(), wt.data_ptr(), cin, ksize, cout,
              _stream())
    return wt


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, ksize: int, in_scale=None, in_shift=None,
                 in_relu: bool = False, out: Optional[torch.Tensor] = None,
                 beta: float = 0.0) -> torch.Tensor:
    """dw [Cin,k*k,Cout] = sum_{n,y,x} x'[n,ci,y+ky-1,x+kx-1] * dy[n,co,y,x] (+ beta*out)."""
    _chk(x, _F32, "wgrad.x", 4)
    _chk(dy, _F32, "wgrad.dy", 4)
    n, cin, h, w = x.shape
    if dy.shape[0] != n or tuple(dy.shape[2:]) != (h, w):
        raise ValueError("wgrad: x and dy must share N,H,W")
    cout = dy.shape[1]
    _prologue("wgrad", in_scale, in_shift, cin)
    if out is None:
        beta = 0.0
    out = _act_out("wgrad", out, (cin, ksize * ksize, cout), (_F32,), _F32, x.device)
    nbytes = _lib.load().lf_conv2d_wgrad_workspace(n, cin, h, w, cout, ksize)
    ws = _workspace(nbytes, x.device)
    _lib.call("lf_conv2d_wgrad_f32", x.data_ptr(), dy.data_ptr(), n, cin, h, w, cout, ksize,
              _ptr(in_scale), _ptr(in_shift), 1 if in_relu else 0, ws.data_ptr(), ws.numel(),
              _stream())
    _lib.call("lf_conv2d_wgrad_reduce_f32", ws.data_ptr(), out.data_ptr(), n, cin, h, w, cout,
              ksize, float(beta), _stream())
    return out


def bn_bwd_wgrad(x: torch.Tensor, g: torch.Tensor, y_bn: torch.Tensor, stats: torch.Tensor, gamma,
                 dgamma, dbeta, relu: bool, ksize: int, dw_out: torch.Tensor, dy_out: torch.Tensor,
                 in_scale=None, in_shift=None, in_relu: bool = False, alpha_nc=None, add_nc=None,
                 plane_g=None, plane_m=None, tile_sums=None) -> torch.Tensor:
    """BatchNormalization backward of g (BN input y_bn) followed by the weight gradient of the
    convolution that produced y_bn from x:  dy = BN'(g) is formed inside the wgrad kernel from
    g and y_bn (and written to dy_out, when given, for the input-gradient convolution); dgamma / dbeta /
    dw_out are filled.  Falls back to the two-kernel route for shapes the fused kernel does not
    take (same results up to rounding)."""
    who = "bn_bwd_wgrad"
    _chk(x, _F32, f"{who}.x", 4)
    n, cin, h, w, cout = _bn_bwd_wgrad_checks(who, _F32, x, g, y_bn, dy_out, dw_out, ksize, in_scale, in_shift,
                                              alpha_nc, add_nc, plane_g, plane_m)
    lib = _lib.load()
    if _NO_FUSED_BN_WGRAD or not lib.lf_conv2d_wgrad_bn_supported(n, cin, h, w, cout, ksize):
        dy = bn_bwd(g, y_bn, stats, gamma, dgamma, dbeta, relu, alpha_nc=alpha_nc, add_nc=add_nc,
                    out=dy_out, plane_g=plane_g, plane_m=plane_m, tile_sums=tile_sums)
        conv2d_wgrad(x, dy, ksize, in_scale, in_shift, in_relu, out=dw_out)
        return dy_out
    coef, _ = _bn_bwd_coef(who, stats, gamma, dgamma, dbeta, relu, n, cout, h * w, x.device, g, y_bn, alpha_nc,
                           add_nc, plane_g, plane_m, tile_sums)
    ws = _workspace(lib.lf_conv2d_wgrad_workspace(n, cin, h, w, cout, ksize), x.device)
    _lib.call("lf_conv2d_wgrad_bn_f32", x.data_ptr(), g.data_ptr(), y_bn.data_ptr(), _ptr(alpha_nc),
              _ptr(add_nc), coef.data_ptr(), 1 if relu else 0, _ptr(dy_out), n, cin, h, w, cout,
              ksize, _ptr(in_scale), _ptr(in_shift), 1 if in_relu else 0, ws.data_ptr(), ws.numel(),
              _stream())
    _lib.call("lf_conv2d_wgrad_reduce_f32", ws.data_ptr(), dw_out.data_ptr(), n, cin, h, w, cout,
              ksize, 0.0, _stream())
    return dy_out


def proj_bwd(x: torch.Tensor, g: torch.Tensor, y_bn: torch.Tensor, stats: torch.Tensor, gamma, dgamma, dbeta,
             w: torch.Tensor, dw_out: torch.Tensor, dx_out: torch.Tensor, dy_scratch: Optional[torch.Tensor] = None,
             in_scale=None, in_shift=None, in_relu: bool = False, plane_g=None) -> torch.Tensor:
    """Backward of a projection shortcut y_bn = conv1x1(x, w) followed by BatchNormalization without ReLU, g being
    the gradient wrt the BatchNorm's output: fills dgamma / dbeta, dw_out [Cin,1,Cout] and dx_out (overwritten: the
    main path's input gradient accumulates onto it afterwards).  One kernel reads x, g and y_bn once and keeps
    dy = BN'(g) on chip (lf_conv2d_proj_bwd_f32); shapes it does not take, and a prologue on x, go through
    bn_bwd_wgrad + conv2d_dgrad_weights + conv2d with dy in dy_scratch (same results up to rounding)."""
    who = "proj_bwd"
    _chk(x, _F32, f"{who}.x", 4)
    n, cin, h, wd, cout = _bn_bwd_wgrad_checks(who, _F32, x, g, y_bn, dy_scratch, dw_out, 1, in_scale, in_shift,
                                               None, None, plane_g, None)
    _chk(w, _F32, f"{who}.w", 3)
    _chk(dx_out, _F32, f"{who}.dx_out", 4)
    if tuple(w.shape) != (cin, 1, cout) or dx_out.shape != x.shape:
        raise ValueError(f"{who}: shape mismatch")
    lib = _lib.load()
    if _NO_FUSED_PROJ_BWD or in_scale is not None or not lib.lf_conv2d_proj_bwd_supported(
            x.data_ptr(), g.data_ptr(), y_bn.data_ptr(), w.data_ptr(), dx_out.data_ptr(), n, cin, h, wd, cout):
        if dy_scratch is None:
            dy_scratch = torch.empty_like(g)
        bn_bwd_wgrad(x, g, y_bn, stats, gamma, dgamma, dbeta, False, 1, dw_out, dy_scratch, in_scale, in_shift,
                     in_relu, plane_g=plane_g)
        return conv2d(dy_scratch, conv2d_dgrad_weights(w, 1), 1, out=dx_out)
    coef, _ = _bn_bwd_coef(who, stats, gamma, dgamma, dbeta, False, n, cout, h * wd, x.device, g, y_bn,
                           plane_g=plane_g)
    ws = _workspace(lib.lf_conv2d_proj_bwd_workspace(n, cin, h, wd, cout), x.device)
    _lib.call("lf_conv2d_proj_bwd_f32", x.data_ptr(), g.data_ptr(), y_bn.data_ptr(), coef.data_ptr(), 0,
              w.data_ptr(), dx_out.data_ptr(), dw_out.data_ptr(), n, cin, h, wd, cout, ws.data_ptr(), ws.numel(),
              _stream())
    return dx_out


def _dw_weights(who: str, w_c9: torch.Tensor, c: int) -> None:
    _chk(w_c9, _F32, f"{who}.w", 2)
    if tuple(w_c9.shape) != (c, 9):
        raise ValueError(f"{who}.w: expected [{c},9], got {tuple(w_c9.shape)}")


def dwconv3x3(x: torch.Tensor, w_c9: torch.Tensor, in_scale=None, in_shift=None, in_relu: bool = False,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Depthwise 3x3 convolution, padding "same": y[n,c] = conv(x'[n,c], w[c]); x' = relu?(x*in_scale[c]+in_shift[c])
    if a prologue is given.  x [N,C,H,W] f32, w_c9 [C,9] (tap = ky*3+kx) -> y [N,C,H,W]."""
    _chk(x, _F32, "dwconv3x3.x", 4)
    n, c, h, w = x.shape
    _dw_weights("dwconv3x3", w_c9, c)
    _prologue("dwconv3x3", in_scale, in_shift, c)
    out = _act_out("dwconv3x3", out, (n, c, h, w), (_F32,), _F32, x.device)
    _lib.call("lf_dwconv3x3_f32", x.data_ptr(), w_c9.data_ptr(), out.data_ptr(), n, c, h, w, _ptr(in_scale),
              _ptr(in_shift), 1 if in_relu else 0, _stream())
    return out


def dwconv3x3_bwd(x: torch.Tensor, w_c9: torch.Tensor, dy: torch.Tensor, dw_out: torch.Tensor,
                  dx_out: Optional[torch.Tensor] = None, accumulate: bool = False, in_scale=None, in_shift=None,
                  in_relu: bool = False):
    """Both gradients of dwconv3x3 in one pass: dw_out [C,9] = sum dy * x' (overwritten, deterministic), and, when
    dx_out is given, dx_out (+)= conv(dy, flipped w), the gradient wrt x' (accumulate: added into dx_out).
    Returns (dw_out, dx_out)."""
    who = "dwconv3x3_bwd"
    _chk(x, _F32, f"{who}.x", 4)
    _chk(dy, _F32, f"{who}.dy", 4)
    n, c, h, w = x.shape
    if dy.shape != x.shape:
        raise ValueError(f"{who}: x and dy must share their shape")
    _dw_weights(who, w_c9, c)
    _dw_weights(f"{who}.dw_out", dw_out, c)
    _prologue(who, in_scale, in_shift, c)
    if dx_out is None and accumulate:
        raise ValueError(f"{who}: accumulate needs dx_out")
    if dx_out is not None:
        _act_out(who, dx_out, (n, c, h, w), (_F32,), None, x.device)
    ws = _workspace(_lib.load().lf_dwconv3x3_bwd_workspace(n, c, h, w), x.device)
    _lib.call("lf_dwconv3x3_bwd_f32", x.data_ptr(), w_c9.data_ptr(), dy.data_ptr(), _ptr(dx_out),
              1 if accumulate else 0, dw_out.data_ptr(), n, c, h, w, _ptr(in_scale), _ptr(in_shift),
              1 if in_relu else 0, ws.data_ptr(), ws.numel(), _stream())
    return dw_out, dx_out


# ---------------------------------------------------------------------------
# non-conv layers
# ---------------------------------------------------------------------------
def input_stage(x_u8: torch.Tensor, aug4: torch.Tensor, mean=None, denom=None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """u8 [N,H,W,3] -> f32 [N,3,H,W] with flip/rotate/contrast (aug4 [N,4]) + Normalization."""
    _chk(x_u8, torch.uint8, "input_stage.x", 4)
    _chk(aug4, _F32, "input_stage.aug", 2)
    n, h, w, c = x_u8.shape
    if c != 3 or tuple(aug4.shape) != (n, 4):
        raise ValueError("input_stage: x must be [N,H,W,3] and aug [N,4]")
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=_F32, device=x_u8.device)
    ws = torch.empty((n, 24), dtype=_F32, device=x_u8.device)
    m = d = None
    if mean is not None:
        m = (_lib.c_float * 3)(*[float(v) for v in mean])
        d = (_lib.c_float * 3)(*[float(v) for v in denom])
    _lib.call("lf_input_stage_f32", x_u8.data_ptr(), out.data_ptr(), n, h, w, aug4.data_ptr(), m, d,
              ws.data_ptr(), _stream())
    return out


def _mix_checks(who: str, lead: torch.Tensor, shaped) -> None:
    """`shaped`: name -> (tensor, expected shape); every one a contiguous float32 tensor on lead's device."""
    for name, (t, shape) in shaped.items():
        if t.dtype != _F32 or not t.is_contiguous() or t.device != lead.device:
            raise ValueError(f"{who}.{name}: a contiguous float32 tensor on {lead.device} expected")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{who}.{name}: expected {tuple(shape)}, got {tuple(t.shape)}")


def input_stage_mix(x_u8: torch.Tensor, aug4: torch.Tensor, mix8: torch.Tensor, mean=None, denom=None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """input_stage with Mixup / CutMix fused (lf_input_stage_mix_f32): every image is blended with the model view of
    its partner, mix8 [N,8] = {partner, w_out, w_in, y0, y1, x0, x1, t} per image (the rule: include/leafhip.h)."""
    if x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3 or not x_u8.is_contiguous() \
            or not x_u8.is_cuda:
        raise ValueError("input_stage_mix.x: a contiguous uint8 [N,H,W,3] tensor on the GPU expected")
    n, h, w, _c = x_u8.shape
    if (mean is None) != (denom is None):
        raise ValueError("input_stage_mix: mean and denom go together")
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=_F32, device=x_u8.device)
    _mix_checks("input_stage_mix", x_u8, {"aug": (aug4, (n, 4)), "mix": (mix8, (n, 8)), "out": (out, (n, 3, h, w))})
    ws = torch.empty((n, 24), dtype=_F32, device=x_u8.device)
    m = d = None
    if mean is not None:
        m = (_lib.c_float * 3)(*[float(v) for v in mean])
        d = (_lib.c_float * 3)(*[float(v) for v in denom])
    _lib.call("lf_input_stage_mix_f32", x_u8.data_ptr(), out.data_ptr(), n, h, w, aug4.data_ptr(), mix8.data_ptr(),
              m, d, ws.data_ptr(), _stream())
    return out


def input_stage_policy(x_u8: torch.Tensor, pol24: torch.Tensor, mean=None, denom=None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The augmentation policy's input stage (lf_input_stage_policy_f32): u8 [N,H,W,3] -> f32 [N,3,H,W], every image
    warped, recoloured and erased by its own row pol24 [N,24] = {a,b,c,d,e,f,g,k, M (3x3), t (3), y0,y1,x0,x1} (the
    rule: include/leafhip.h), then normalised with mean / denom as pack_hwc_u8_to_nchw_f32 does it."""
    if x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3 or not x_u8.is_contiguous() \
            or not x_u8.is_cuda:
        raise ValueError("input_stage_policy.x: a contiguous uint8 [N,H,W,3] tensor on the GPU expected")
    n, h, w, _c = x_u8.shape
    if (mean is None) != (denom is None):
        raise ValueError("input_stage_policy: mean and denom go together")
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=_F32, device=x_u8.device)
    _mix_checks("input_stage_policy", x_u8, {"pol": (pol24, (n, 24)), "out": (out, (n, 3, h, w))})
    m = d = None
    if mean is not None:
        m = (_lib.c_float * 3)(*[float(v) for v in mean])
        d = (_lib.c_float * 3)(*[float(v) for v in denom])
    _lib.call("lf_input_stage_policy_f32", x_u8.data_ptr(), out.data_ptr(), n, h, w, pol24.data_ptr(), m, d,
              _stream())
    return out


def mix_targets(y: torch.Tensor, mix8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mixed targets out[i] = y[p] + t (y[i] - y[p]) with p, t from mix8 [N,8] (lf_mix_targets_f32), out of place."""
    if y.dim() != 2 or not y.is_cuda:
        raise ValueError(f"mix_targets.y: [N,C] on the GPU expected, got {tuple(y.shape)} on {y.device}")
    n, c = y.shape
    if out is None:
        out = torch.empty_like(y)
    _mix_checks("mix_targets", y, {"y": (y, (n, c)), "mix": (mix8, (n, 8)), "out": (out, (n, c))})
    if abs(out.data_ptr() - y.data_ptr()) < 4 * n * c:
        raise ValueError("mix_targets: out must not overlap y (a row is also read as its partner's partner)")
    _lib.call("lf_mix_targets_f32", y.data_ptr(), mix8.data_ptr(), out.data_ptr(), n, c, _stream())
    return out


TTA_MAX_VIEWS = 16


def _host_f32(who: str, values, shape) -> "np.ndarray":
    """A host array of float32 in C order with the given shape (-1: any), from an array, a list or a CPU tensor."""
    import numpy as np
    if isinstance(values, torch.Tensor):
        if values.is_cuda:
            raise ValueError(f"{who}: host values expected (they travel as kernel arguments), got a tensor on "
                             f"{values.device}")
        values = values.numpy()
    a = np.ascontiguousarray(np.asarray(values), dtype=np.float32)
    if a.ndim != len(shape) or any(s not in (-1, d) for s, d in zip(shape, a.shape)):
        raise ValueError(f"{who}: expected shape {tuple(shape)}, got {a.shape}")
    return a


def tta_views(x_u8: torch.Tensor, rows, mean=None, denom=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """v views of every image in one launch (lf_tta_views_f32; the rule: include/leafhip.h): x_u8 uint8 [N,H,W,3] on
    the GPU, rows [v,6] = {flip, cos, sin, zoom, dy, dx} per view on the HOST -> f32 [N*v,3,H,W], row i*v + k the
    view k of image i, normalised with mean / denom as pack_hwc_u8_to_nchw_f32 does it."""
    if not isinstance(x_u8, torch.Tensor) or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3 \
            or not x_u8.is_contiguous() or not x_u8.is_cuda:
        raise ValueError("tta_views.x: a contiguous uint8 [N,H,W,3] tensor on the GPU expected")
    n, h, w, _c = x_u8.shape
    r = _host_f32("tta_views.rows", rows, (-1, 6))
    v = r.shape[0]
    if not 1 <= v <= TTA_MAX_VIEWS:
        raise ValueError(f"tta_views: {v} views (1..{TTA_MAX_VIEWS})")
    if (mean is None) != (denom is None):
        raise ValueError("tta_views: mean and denom go together")
    if out is None:
        out = torch.empty((n * v, 3, h, w), dtype=_F32, device=x_u8.device)
    _mix_checks("tta_views", x_u8, {"out": (out, (n * v, 3, h, w))})
    m = d = None
    if mean is not None:
        m = (_lib.c_float * 3)(*[float(t) for t in mean])
        d = (_lib.c_float * 3)(*[float(t) for t in denom])
    _lib.call("lf_tta_views_f32", x_u8.data_ptr(), out.data_ptr(), n, h, w, r.ctypes.data, v, m, d, _stream())
    return out


def tta_combine(probs: torch.Tensor, v: int, weights=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The v probability rows of every image folded into one (lf_tta_combine_f32): probs f32 [N*v,C] image-major,
    weights v host floats (None: all 1) -> (out [N,C] the weighted mean, top [N] int32 its argmax, agree [N] int32
    the number of counted views whose own argmax is top)."""
    _chk(probs, _F32, "tta_combine.probs", 2)
    rows, c = probs.shape
    v = int(v)
    if not 1 <= v <= TTA_MAX_VIEWS:
        raise ValueError(f"tta_combine: {v} views (1..{TTA_MAX_VIEWS})")
    if rows == 0 or rows % v:
        raise ValueError(f"tta_combine.probs: {rows} rows are not a positive multiple of v={v}")
    wt = None if weights is None else _host_f32("tta_combine.weights", weights, (v,))
    n = rows // v
    out = torch.empty((n, c), dtype=_F32, device=probs.device)
    top = torch.empty((n,), dtype=torch.int32, device=probs.device)
    agree = torch.empty((n,), dtype=torch.int32, device=probs.device)
    _lib.call("lf_tta_combine_f32", probs.data_ptr(), None if wt is None else wt.ctypes.data, v, out.data_ptr(),
              top.data_ptr(), agree.data_ptr(), n, c, _stream())
    return out, top, agree


CALIB_MAX_BETAS = 8
CALIB_MAX_BINS = 64
CALIB_MAX_CLASSES = 4096
CALIB_SUMS = ("nll", "g", "h", "brier", "conf")
CALIB_STATS_WAVES = 1024   # the most waves a calib_stats launch runs: beyond that many rows a wave takes several


def _calib_probs(who: str, probs: torch.Tensor) -> Tuple[int, int]:
    _chk(probs, _F32, f"{who}.probs", 2)
    n, c = probs.shape
    if n == 0 or not 1 <= c <= CALIB_MAX_CLASSES:
        raise ValueError(f"{who}.probs: [N,C] with N > 0 and 1 <= C <= {CALIB_MAX_CLASSES} expected, got "
                         f"{tuple(probs.shape)}")
    return n, c


def _calib_beta(who: str, beta) -> float:
    import math
    b = float(beta)
    if not (math.isfinite(b) and b > 0.0):
        raise ValueError(f"{who}: an inverse temperature must be finite and positive, got {beta!r}")
    return b


def calib_stats(probs: torch.Tensor, labels: torch.Tensor, betas, bins: int = 15, confusion: bool = True) -> dict:
    """What probability rows and their labels say about each inverse temperature of `betas` (lf_calib_stats; the
    rule: include/leafhip.h): probs f32 [N,C] and labels int32 [N] on the GPU, betas 1..8 host floats.  Returns host
    numpy arrays: betas [K]; nll, g, h, brier, conf f64 [K] (sums over the rows with a label in [0, C)); bin_conf f64
    [K,bins], bin_count and bin_correct int64 [K,bins]; pred int32 [N]; confusion int64 [C,C] ([true][pred]) or
    None; and the ints n (rows counted), correct, skipped and bins.  One device-to-host sync."""
    import numpy as np
    n, c = _calib_probs("calib_stats", probs)
    _chk(labels, torch.int32, "calib_stats.labels", 1)
    if labels.shape[0] != n or labels.device != probs.device:
        raise ValueError(f"calib_stats.labels: expected [{n}] on {probs.device}, got {tuple(labels.shape)} on "
                         f"{labels.device}")
    bt = np.ascontiguousarray(np.atleast_1d(np.asarray(betas, dtype=np.float64)))
    if bt.ndim != 1 or not 1 <= bt.shape[0] <= CALIB_MAX_BETAS:
        raise ValueError(f"calib_stats.betas: 1..{CALIB_MAX_BETAS} values expected, got shape {bt.shape}")
    for b in bt:
        _calib_beta("calib_stats.betas", b)
    k, bins = int(bt.shape[0]), int(bins)
    if not 1 <= bins <= CALIB_MAX_BINS:
        raise ValueError(f"calib_stats: bins={bins} (1..{CALIB_MAX_BINS})")
    per = len(CALIB_SUMS) + bins
    sums = torch.empty((k, per), dtype=torch.float64, device=probs.device)
    counts = torch.empty((k * 2 * bins + 2,), dtype=torch.int32, device=probs.device)
    pred = torch.empty((n,), dtype=torch.int32, device=probs.device)
    cm = torch.empty((c, c), dtype=torch.int32, device=probs.device) if confusion else None
    ws = _workspace(_lib.load().lf_calib_stats_workspace(n, k, bins), probs.device)
    _lib.call("lf_calib_stats", probs.data_ptr(), labels.data_ptr(), n, c, bt.ctypes.data, k, bins, sums.data_ptr(),
              counts.data_ptr(), pred.data_ptr(), _ptr(cm), ws.data_ptr(), ws.numel(), _stream())
    sums_h, counts_h = sums.cpu().numpy(), counts.cpu().numpy().astype(np.int64)
    per_bin = counts_h[:k * 2 * bins].reshape(k, 2, bins)
    out = {name: sums_h[:, j].copy() for j, name in enumerate(CALIB_SUMS)}
    skipped = int(counts_h[-1])
    out.update(betas=bt.copy(), bin_conf=sums_h[:, len(CALIB_SUMS):].copy(), bin_count=per_bin[:, 0].copy(),
               bin_correct=per_bin[:, 1].copy(), pred=pred.cpu().numpy(),
               confusion=None if cm is None else cm.cpu().numpy().astype(np.int64),
               n=n - skipped, correct=int(counts_h[-2]), skipped=skipped, bins=bins)
    return out


def calib_apply(probs: torch.Tensor, beta, out: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The rows at inverse temperature beta (lf_calib_apply_f32): probs f32 [N,C] on the GPU -> (out f32 [N,C] =
    softmax(beta ln max(probs, FLT_MIN)), conf f32 [N] its row maximum, top int32 [N] the argmax of the INPUT row,
    lowest index on ties).  `out` may be probs itself (in place); any other overlap is refused."""
    n, c = _calib_probs("calib_apply", probs)
    b = _calib_beta("calib_apply.beta", beta)
    if out is None:
        out = torch.empty_like(probs)
    _mix_checks("calib_apply", probs, {"out": (out, (n, c))})
    lo, hi = out.data_ptr(), probs.data_ptr()
    if lo != hi and abs(lo - hi) < 4 * n * c:
        raise ValueError("calib_apply: out overlaps probs without being probs (in place means out is probs)")
    conf = torch.empty((n,), dtype=_F32, device=probs.device)
    top = torch.empty((n,), dtype=torch.int32, device=probs.device)
    _lib.call("lf_calib_apply_f32", probs.data_ptr(), _lib.c_double(b), out.data_ptr(), conf.data_ptr(),
              top.data_ptr(), n, c, _stream())
    return out, conf, top


CONFORMAL_MAX_CLASSES = 256
CONFORMAL_KINDS = ("lac", "aps", "raps")   # LF_CONFORMAL_LAC, _APS, _RAPS
CONFORMAL_WAVES = 8192     # the most waves a conformal launch runs: beyond that many rows a wave takes several
CONFORMAL_GLOBALS = ("rows", "skipped", "covered", "size_sum")


def _conformal_args(who: str, probs: torch.Tensor, u, kind, lam, kreg) -> Tuple[int, int, int, float, int]:
    """The checks both conformal wrappers make -> (n, c, kind number, lambda, kreg)."""
    import math
    _chk(probs, _F32, f"{who}.probs", 2)
    n, c = probs.shape
    if n == 0 or not 1 <= c <= CONFORMAL_MAX_CLASSES:
        raise ValueError(f"{who}.probs: [N,C] with N > 0 and 1 <= C <= {CONFORMAL_MAX_CLASSES} expected, got "
                         f"{tuple(probs.shape)}")
    if u is not None:
        _chk(u, _F32, f"{who}.u", 1)
        if u.shape[0] != n or u.device != probs.device:
            raise ValueError(f"{who}.u: expected [{n}] on {probs.device}, got {tuple(u.shape)} on {u.device}")
    if kind not in CONFORMAL_KINDS:
        raise ValueError(f"{who}: unknown score {kind!r}: one of {', '.join(CONFORMAL_KINDS)}")
    lam, kreg = float(lam), int(kreg)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"{who}: lambda must be finite and >= 0, got {lam!r}")
    if kreg < 0:
        raise ValueError(f"{who}: kreg must be >= 0, got {kreg}")
    return n, c, CONFORMAL_KINDS.index(kind), lam, kreg


def _conformal_labels(who: str, labels: torch.Tensor, probs: torch.Tensor) -> None:
    _chk(labels, torch.int32, f"{who}.labels", 1)
    if labels.shape[0] != probs.shape[0] or labels.device != probs.device:
        raise ValueError(f"{who}.labels: expected [{probs.shape[0]}] on {probs.device}, got {tuple(labels.shape)} on "
                         f"{labels.device}")


def conformal_scores(probs: torch.Tensor, labels: torch.Tensor, u: Optional[torch.Tensor] = None, kind: str = "aps",
                     lam: float = 0.0, kreg: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The conformity score of every row's label (lf_conformal_scores; the rule: include/leafhip.h "Conformal"):
    probs f32 [N,C], labels int32 [N] and u f32 [N] (None: 1.0 for every row) on the GPU -> (score f64 [N], rank
    int32 [N] = the classes that stand before the label).  A label outside [0, C) gives (NaN, -1).  No sync."""
    n, c, k, lam, kreg = _conformal_args("conformal_scores", probs, u, kind, lam, kreg)
    _conformal_labels("conformal_scores", labels, probs)
    score = torch.empty((n,), dtype=torch.float64, device=probs.device)
    rank = torch.empty((n,), dtype=torch.int32, device=probs.device)
    _lib.call("lf_conformal_scores", probs.data_ptr(), labels.data_ptr(), _ptr(u), n, c, k, _lib.c_double(lam), kreg,
              score.data_ptr(), rank.data_ptr(), _stream())
    return score, rank


def conformal_sets(probs: torch.Tensor, qhat: torch.Tensor, u: Optional[torch.Tensor] = None, kind: str = "aps",
                   lam: float = 0.0, kreg: int = 0, force_top: bool = True, labels: Optional[torch.Tensor] = None,
                   stats: bool = False) -> Tuple[torch.Tensor, torch.Tensor, Optional[dict]]:
    """The prediction sets at the thresholds qhat (lf_conformal_sets): probs f32 [N,C], qhat f64 [C] (one threshold
    per class; a marginal one repeated), u f32 [N] or None and labels int32 [N] or None on the GPU -> (member uint8
    [N,C], size int32 [N], stats).  With `stats` (needs labels; one device-to-host sync) the counters over the rows
    whose label lies in [0, C) as host values: the ints rows, skipped, covered and size_sum, size_hist int64 [C+1],
    and class_rows, class_covered, class_size_sum int64 [C]; None without."""
    n, c, k, lam, kreg = _conformal_args("conformal_sets", probs, u, kind, lam, kreg)
    _chk(qhat, torch.float64, "conformal_sets.qhat", 1)
    if qhat.shape[0] != c or qhat.device != probs.device:
        raise ValueError(f"conformal_sets.qhat: expected [{c}] on {probs.device}, got {tuple(qhat.shape)} on "
                         f"{qhat.device}")
    if labels is not None:
        _conformal_labels("conformal_sets", labels, probs)
    elif stats:
        raise ValueError("conformal_sets: stats need labels")
    member = torch.empty((n, c), dtype=torch.uint8, device=probs.device)
    size = torch.empty((n,), dtype=torch.int32, device=probs.device)
    g = len(CONFORMAL_GLOBALS)
    counters = torch.empty((g + c + 1 + 3 * c,), dtype=torch.int64, device=probs.device) if stats else None
    _lib.call("lf_conformal_sets", probs.data_ptr(), _ptr(u), qhat.data_ptr(), n, c, k, _lib.c_double(lam), kreg,
              int(bool(force_top)), _ptr(labels), member.data_ptr(), size.data_ptr(), _ptr(counters), _stream())
    if counters is None:
        return member, size, None
    h = counters.cpu().numpy()
    per = h[g + c + 1:].reshape(c, 3)
    out = {name: int(h[j]) for j, name in enumerate(CONFORMAL_GLOBALS)}
    out.update(size_hist=h[g:g + c + 1].copy(), class_rows=per[:, 0].copy(), class_covered=per[:, 1].copy(),
               class_size_sum=per[:, 2].copy())
    return member, size, out


NOVELTY_MAX_DIM = 256
NOVELTY_DIM_STEP = 16
NOVELTY_MAX_CLASSES = 4096
NOVELTY_STATE = (("count", torch.int64), ("skipped", torch.int64), ("sum", torch.float64), ("gram", torch.float64))


def novelty_dim_ok(d: int) -> bool:
    """Whether the novelty kernels take feature rows of d floats."""
    return NOVELTY_DIM_STEP <= d <= NOVELTY_MAX_DIM and d % NOVELTY_DIM_STEP == 0


def _novelty_feat(who: str, feat: torch.Tensor) -> Tuple[int, int]:
    _chk(feat, _F32, f"{who}.feat", 2)
    n, d = feat.shape
    if n == 0 or not novelty_dim_ok(d):
        raise ValueError(f"{who}.feat: [N,D] with N > 0 and D a multiple of {NOVELTY_DIM_STEP} in "
                         f"{NOVELTY_DIM_STEP}..{NOVELTY_MAX_DIM} expected, got {tuple(feat.shape)}")
    return n, d


def _novelty_classes(who: str, c) -> int:
    c = int(c)
    if not 1 <= c <= NOVELTY_MAX_CLASSES:
        raise ValueError(f"{who}: {c} classes (1..{NOVELTY_MAX_CLASSES})")
    return c


def feat_moments(feat: torch.Tensor, labels: torch.Tensor, num_classes: int, state: Optional[dict] = None) -> dict:
    """The float64 sums of a Mahalanobis fit, added into `state` (lf_feat_moments; the rule: include/leafhip.h): feat
    f32 [N,D] and labels int32 [N] on the GPU.  state: {"count" int64 [C], "skipped" int64 [1], "sum" f64 [C,D],
    "gram" f64 [D,D]} on feat's device, created zeroed when None; returned.  A row whose label lies outside [0, C)
    counts in `skipped` alone.  No sync."""
    n, d = _novelty_feat("feat_moments", feat)
    c = _novelty_classes("feat_moments.num_classes", num_classes)
    _chk(labels, torch.int32, "feat_moments.labels", 1)
    if labels.shape[0] != n or labels.device != feat.device:
        raise ValueError(f"feat_moments.labels: expected [{n}] on {feat.device}, got {tuple(labels.shape)} on "
                         f"{labels.device}")
    shapes = {"count": (c,), "skipped": (1,), "sum": (c, d), "gram": (d, d)}
    if state is None:
        state = {k: torch.zeros(shapes[k], dtype=dt, device=feat.device) for k, dt in NOVELTY_STATE}
    if not isinstance(state, dict):
        raise TypeError(f"feat_moments.state: a dict of {', '.join(k for k, _dt in NOVELTY_STATE)} expected")
    for k, dt in NOVELTY_STATE:
        t = state.get(k)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"feat_moments.state: no tensor {k!r}")
        if t.dtype != dt:
            raise TypeError(f"feat_moments.state.{k}: expected {dt}, got {t.dtype}")
        if tuple(t.shape) != shapes[k] or not t.is_contiguous() or t.device != feat.device:
            raise ValueError(f"feat_moments.state.{k}: a contiguous {shapes[k]} tensor on {feat.device} expected, got "
                             f"{tuple(t.shape)} on {t.device}")
    _lib.call("lf_feat_moments", feat.data_ptr(), labels.data_ptr(), n, d, c, state["count"].data_ptr(),
              state["skipped"].data_ptr(), state["sum"].data_ptr(), state["gram"].data_ptr(), _stream())
    return state


def maha_score(feat: torch.Tensor, mu0: torch.Tensor, W: torch.Tensor, M: torch.Tensor, want_d2: bool = False
               ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Squared distance to the nearest whitened class mean (lf_maha_score_f32; the rule: include/leafhip.h): feat f32
    [N,D], mu0 f32 [D], W f32 [D,D] row-major and M f32 [C,D] on the GPU -> (score f32 [N] = min_c |W (f - mu0) -
    M_c|^2, nearest int32 [N] the lowest class attaining it, d2 f32 [N,C] with want_d2 else None).  A non-finite
    distance reads as +inf; a row with no finite one gets (+inf, 0)."""
    n, d = _novelty_feat("maha_score", feat)
    _chk(M, _F32, "maha_score.M", 2)
    c = _novelty_classes("maha_score.M", M.shape[0])
    _mix_checks("maha_score", feat, {"mu0": (mu0, (d,)), "W": (W, (d, d)), "M": (M, (c, d))})
    score = torch.empty((n,), dtype=_F32, device=feat.device)
    nearest = torch.empty((n,), dtype=torch.int32, device=feat.device)
    d2 = torch.empty((n, c), dtype=_F32, device=feat.device) if want_d2 else None
    _lib.call("lf_maha_score_f32", feat.data_ptr(), mu0.data_ptr(), W.data_ptr(), M.data_ptr(), n, d, c, _ptr(d2),
              score.data_ptr(), nearest.data_ptr(), _stream())
    return score, nearest, d2


KNN_MAX_K = 32
KNN_MAX_SEGMENTS = 64


def knn_geometry(nq: int, ng: int) -> Tuple[int, int, int]:
    """How lf_knn_topk_f32 walks nq queries against ng gallery rows when `segments` is left to it, from the library:
    (queries per workgroup, segments the gallery is cut into, gallery rows per segment)."""
    lib = _lib.load()
    nq, ng = int(nq), int(ng)
    segments = lib.lf_knn_segments(nq, ng)
    if segments < 1:
        raise ValueError(f"knn_geometry: nq={nq}, ng={ng} (each >= 1 and below 2^31)")
    return lib.lf_knn_query_tile(), segments, -(-ng // segments)


def _knn_rows(who: str, t: torch.Tensor) -> Tuple[int, int]:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.LeafHipError(f"{who}: expected a CUDA(HIP) tensor — there is no CPU path")
    if t.dtype != _F32 or t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{who}: a contiguous float32 [N,D] tensor expected, got {t.dtype} {tuple(t.shape)}"
                         f"{'' if t.is_contiguous() else ' (not contiguous)'}")
    n, d = t.shape
    if n == 0 or n >= 1 << 31 or not novelty_dim_ok(d):
        raise ValueError(f"{who}: [N,D] with 1 <= N < 2^31 and D a multiple of {NOVELTY_DIM_STEP} in "
                         f"{NOVELTY_DIM_STEP}..{NOVELTY_MAX_DIM} expected, got {tuple(t.shape)}")
    return n, d


def knn_topk(queries: torch.Tensor, gallery: torch.Tensor, k: int, exclude: Optional[torch.Tensor] = None,
             segments: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k gallery rows nearest to each query (lf_knn_topk_f32; the rule: include/leafhip.h): queries f32 [nq,D] and
    gallery f32 [ng,D] on the GPU -> (d2 f32 [nq,k], idx int32 [nq,k]), each row ascending by (d2, index), padded with
    (+inf, -1) when fewer than k rows are eligible.  exclude int32 [nq]: the gallery row query i must not return, -1
    for none.  segments: into how many runs the gallery is cut (None: knn_geometry's choice); the result does not
    depend on it.  The distance matrix is never written.  No sync."""
    nq, d = _knn_rows("knn_topk.queries", queries)
    ng, dg = _knn_rows("knn_topk.gallery", gallery)
    if dg != d or gallery.device != queries.device:
        raise ValueError(f"knn_topk.gallery: [ng,{d}] on {queries.device} expected, got {tuple(gallery.shape)} on "
                         f"{gallery.device}")
    if gallery.data_ptr() % 16:
        raise ValueError("knn_topk.gallery: must start on a 16-byte boundary")
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"knn_topk: k={k} (1..{KNN_MAX_K})")
    if exclude is not None:
        if not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.int32 or exclude.dim() != 1 \
                or exclude.shape[0] != nq or not exclude.is_contiguous() or exclude.device != queries.device:
            raise ValueError(f"knn_topk.exclude: a contiguous int32 [{nq}] tensor on {queries.device} expected")
    lib = _lib.load()
    segments = lib.lf_knn_segments(nq, ng) if segments is None else int(segments)
    if not 1 <= segments <= KNN_MAX_SEGMENTS:
        raise ValueError(f"knn_topk: segments={segments} (1..{KNN_MAX_SEGMENTS})")
    nbytes = int(lib.lf_knn_topk_workspace(nq, ng, k, segments))
    ws = _workspace(nbytes, queries.device, slot=4)
    d2 = torch.empty((nq, k), dtype=_F32, device=queries.device)
    idx = torch.empty((nq, k), dtype=torch.int32, device=queries.device)
    _lib.call("lf_knn_topk_f32", queries.data_ptr(), gallery.data_ptr(), nq, ng, d, k, _ptr(exclude), segments,
              d2.data_ptr(), idx.data_ptr(), ws.data_ptr(), nbytes, _stream())
    return d2, idx


TSNE_MAX_POINTS = 16384    # lf_tsne_max_points(): P is 1 GiB there


def _tsne_tensor(who: str, t: torch.Tensor, dtype, shape, device=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.LeafHipError(f"{who}: expected a CUDA(HIP) tensor — there is no CPU path")
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{who}: a contiguous {dtype} {list(shape)} tensor expected, got {t.dtype} {tuple(t.shape)}"
                         f"{'' if t.is_contiguous() else ' (not contiguous)'}")
    if device is not None and t.device != device:
        raise ValueError(f"{who}: expected on {device}, got {t.device}")
    return t


def _tsne_square(who: str, t: torch.Tensor, least: int) -> int:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.LeafHipError(f"{who}: expected a CUDA(HIP) tensor — there is no CPU path")
    if t.dim() != 2 or t.shape[0] != t.shape[1] or not least <= t.shape[0] <= TSNE_MAX_POINTS:
        raise ValueError(f"{who}: [n,n] with {least} <= n <= {TSNE_MAX_POINTS} expected, got {tuple(t.shape)}")
    n = int(t.shape[0])
    _tsne_tensor(who, t, _F32, (n, n))
    if t.data_ptr() % 16:
        raise ValueError(f"{who}: must start on a 16-byte boundary")
    return n


def tsne_perplexity(d2: torch.Tensor, perplexity: float, out: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The conditional affinity rows of t-SNE (lf_tsne_perplexity_f32; the rule: include/leafhip.h "Embedding map"):
    d2 f32 [n,n] squared distances -> (p f32 [n,n] with p[i,i] = 0, beta f64 [n], evals int32 [n]).  out: where p
    goes; None or d2 itself: in place, into d2.  No sync."""
    n = _tsne_square("tsne_perplexity.d2", d2, 2)
    perplexity = float(perplexity)
    if not (perplexity >= 1.0 and perplexity < float("inf")):
        raise ValueError(f"tsne_perplexity: perplexity={perplexity} (finite, >= 1)")
    p = d2 if out is None else out
    if p is not d2:
        _tsne_tensor("tsne_perplexity.out", p, _F32, (n, n), d2.device)
    beta = torch.empty((n,), dtype=torch.float64, device=d2.device)
    evals = torch.empty((n,), dtype=torch.int32, device=d2.device)
    _lib.call("lf_tsne_perplexity_f32", d2.data_ptr(), n, perplexity, p.data_ptr(), beta.data_ptr(), evals.data_ptr(),
              _stream())
    return p, beta, evals


def tsne_symmetrize(p: torch.Tensor) -> torch.Tensor:
    """P = (p + p^T) / 2n in f32, in place (lf_tsne_symmetrize_f32): p f32 [n,n].  Returns p.  No sync."""
    n = _tsne_square("tsne_symmetrize.p", p, 1)
    _lib.call("lf_tsne_symmetrize_f32", p.data_ptr(), n, _stream())
    return p


def tsne_forces(p: torch.Tensor, y: torch.Tensor, want_kl: bool = False, out: Optional[dict] = None) -> dict:
    """The all-pairs sums of one t-SNE iteration (lf_tsne_forces_f32): P f32 [n,n] and the map y f32 [n,2] ->
    {"attr" f32 [n,2], "rep" f32 [n,2], "z" f64 [n], "kl" f64 [n,2] (want_kl; else None)}.  out: such a dict to
    write into (the loop reuses one).  P is read once; nothing of size n^2 is written.  No sync."""
    n = _tsne_square("tsne_forces.p", p, 2)
    dev = p.device
    _tsne_tensor("tsne_forces.y", y, _F32, (n, 2), dev)
    if y.data_ptr() % 16:
        raise ValueError("tsne_forces.y: must start on a 16-byte boundary")
    if out is None:
        out = {"attr": torch.empty((n, 2), dtype=_F32, device=dev), "rep": torch.empty((n, 2), dtype=_F32, device=dev),
               "z": torch.empty((n,), dtype=torch.float64, device=dev), "kl": None}
    res = dict(out)
    _tsne_tensor("tsne_forces.attr", res["attr"], _F32, (n, 2), dev)
    _tsne_tensor("tsne_forces.rep", res["rep"], _F32, (n, 2), dev)
    _tsne_tensor("tsne_forces.z", res["z"], torch.float64, (n,), dev)
    if want_kl:
        if res.get("kl") is None:
            res["kl"] = torch.empty((n, 2), dtype=torch.float64, device=dev)
        _tsne_tensor("tsne_forces.kl", res["kl"], torch.float64, (n, 2), dev)
    else:
        res["kl"] = None
    _lib.call("lf_tsne_forces_f32", p.data_ptr(), y.data_ptr(), n, res["attr"].data_ptr(), res["rep"].data_ptr(),
              res["z"].data_ptr(), _ptr(res["kl"]), _stream())
    return res


def tsne_step(y: torch.Tensor, vel: torch.Tensor, gain: torch.Tensor, forces: dict, exaggeration: float, eta: float,
              momentum: float, sum_p: Optional[float] = None, kl_out: Optional[torch.Tensor] = None
              ) -> Optional[torch.Tensor]:
    """One gradient step of t-SNE with gains, momentum and recentring, in place on y, vel, gain f32 [n,2]
    (lf_tsne_step_f32), from tsne_forces' sums AT THIS y.  When the forces carry "kl" and sum_p (the float64 sum of
    P) is given, the Kullback-Leibler divergence at the y the forces were taken at goes to kl_out f64 [1] (made when
    None) and is returned, on the device.  One workgroup; no sync."""
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("tsne_step.y: a float32 [n,2] tensor expected")
    n = int(y.shape[0])
    if not 2 <= n <= TSNE_MAX_POINTS:
        raise ValueError(f"tsne_step: n={n} (2..{TSNE_MAX_POINTS})")
    _tsne_tensor("tsne_step.y", y, _F32, (n, 2))
    dev = y.device
    for name, t in (("vel", vel), ("gain", gain), ("attr", forces["attr"]), ("rep", forces["rep"])):
        _tsne_tensor(f"tsne_step.{name}", t, _F32, (n, 2), dev)
    _tsne_tensor("tsne_step.z", forces["z"], torch.float64, (n,), dev)
    kl = forces.get("kl") if sum_p is not None else None
    if kl is not None:
        _tsne_tensor("tsne_step.kl", kl, torch.float64, (n, 2), dev)
        if kl_out is None:
            kl_out = torch.empty((1,), dtype=torch.float64, device=dev)
        _tsne_tensor("tsne_step.kl_out", kl_out, torch.float64, (1,), dev)
    else:
        kl_out = None
    _lib.call("lf_tsne_step_f32", y.data_ptr(), vel.data_ptr(), gain.data_ptr(), forces["attr"].data_ptr(),
              forces["rep"].data_ptr(), forces["z"].data_ptr(), n, float(exaggeration), float(eta), float(momentum),
              _ptr(kl), 0.0 if sum_p is None else float(sum_p), _ptr(kl_out), _stream())
    return kl_out


DHASH_VARIANTS = (1, 2, 4, 8)
DHASH_MIN_SIDE, DHASH_MAX_SIDE = 9, 4096


def dhash128(x_u8: torch.Tensor, variants: int = 2) -> torch.Tensor:
    """128-bit difference hashes of a batch (lf_dhash128_u8; the rule: include/leafhip.h): x_u8 uint8 [N,H,W,3] on the
    GPU with 9 <= H, W <= 4096 -> int32 [N,V,4], variant s < V the signature of the flipped / turned cell grid (1: the
    mirrored image)."""
    if not isinstance(x_u8, torch.Tensor) or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3 \
            or not x_u8.is_contiguous() or not x_u8.is_cuda:
        raise ValueError("dhash128.x: a contiguous uint8 [N,H,W,3] tensor on the GPU expected")
    n, h, w, _c = x_u8.shape
    if not (DHASH_MIN_SIDE <= h <= DHASH_MAX_SIDE and DHASH_MIN_SIDE <= w <= DHASH_MAX_SIDE):
        raise ValueError(f"dhash128.x: H={h}, W={w} (each {DHASH_MIN_SIDE}..{DHASH_MAX_SIDE})")
    if variants not in DHASH_VARIANTS:
        raise ValueError(f"dhash128: variants={variants!r} (one of {DHASH_VARIANTS})")
    sig = torch.empty((n, int(variants), 4), dtype=torch.int32, device=x_u8.device)
    if n:
        _lib.call("lf_dhash128_u8", x_u8.data_ptr(), sig.data_ptr(), n, h, w, int(variants), _stream())
    return sig


def hamming_pairs_geometry(na: int, nb: int) -> Tuple[int, int, int, int]:
    """How lf_hamming_pairs_* walk na rows against nb columns, from the library: (rows of `a` per workgroup, columns of
    `b` staged at a time, chunks the columns are cut into, columns per chunk — whole tiles)."""
    lib = _lib.load()
    rows, tile, chunks = lib.lf_hamming_pairs_rows(), lib.lf_hamming_pairs_tile(), lib.lf_hamming_pairs_chunks(na, nb)
    tiles = -(-nb // tile)
    return rows, tile, chunks, -(-tiles // chunks) * tile


def _signatures(who: str, sig: torch.Tensor) -> Tuple[int, int]:
    _chk(sig, torch.int32, who, 3)
    n, v, words = sig.shape
    if words != 4 or v not in DHASH_VARIANTS:
        raise ValueError(f"{who}: int32 [n,V,4] with V one of {DHASH_VARIANTS} expected, got {tuple(sig.shape)}")
    return n, v


def hamming_pairs(sig: torch.Tensor, threshold: int, other: Optional[torch.Tensor] = None,
                  max_pairs: int = 1 << 24) -> torch.Tensor:
    """All pairs of signatures within `threshold` bits (lf_hamming_pairs_count -> scan -> lf_hamming_pairs_fill; the
    rule: include/leafhip.h): sig int32 [n,V,4] on the GPU -> int32 [m,4] rows {i, j, distance, s} in ascending (i, j)
    order, the distance the minimum over the V variants of column j and s the lowest variant reaching it.  other=None:
    rows are variant 0 of `sig` itself and only i < j is reported; else the rows are variant 0 of `other` [na,Va,4].
    Raises ValueError naming the total when more than `max_pairs` pairs match, before anything of that size is
    allocated.  One device-to-host sync (the total)."""
    nb, v = _signatures("hamming_pairs.sig", sig)
    threshold = int(threshold)
    if not 0 <= threshold <= 128:
        raise ValueError(f"hamming_pairs: threshold={threshold} (0..128)")
    rows = sig if other is None else other
    if other is not None:
        _signatures("hamming_pairs.other", other)
        if other.device != sig.device:
            raise ValueError(f"hamming_pairs.other: expected a tensor on {sig.device}, got {other.device}")
    na, va = rows.shape[0], rows.shape[1]
    out = torch.empty((0, 4), dtype=torch.int32, device=sig.device)
    if na == 0 or nb == 0:
        return out
    lib = _lib.load()
    chunks = lib.lf_hamming_pairs_chunks(na, nb)
    counts = torch.empty((na, chunks), dtype=torch.int32, device=sig.device)
    args = (rows.data_ptr(), 4 * va, na, sig.data_ptr(), nb, v, threshold, 1 if other is None else 0)
    _lib.call("lf_hamming_pairs_count", *args, counts.data_ptr(), chunks, _stream())
    ends = torch.cumsum(counts.view(-1), 0, dtype=torch.int64)
    total = int(ends[-1].item())
    if total > int(max_pairs):
        raise ValueError(f"hamming_pairs: {total} pairs within {threshold} bits, more than max_pairs={int(max_pairs)}"
                         f" (lower the threshold, or raise max_pairs)")
    if total == 0:
        return out
    offsets = (ends - counts.view(-1)).contiguous()
    out = torch.empty((total, 4), dtype=torch.int32, device=sig.device)
    _lib.call("lf_hamming_pairs_fill", *args, offsets.data_ptr(), chunks, out.data_ptr(), _stream())
    return out


def scale_shift_act(x, scale, shift, relu: bool, out=None):
    _chk(x, _F32, "scale_shift_act.x", 4)
    n, c, h, w = x.shape
    for t in (scale, shift):
        _chk(t, _F32, "scale_shift_act.scale/shift", 1)
        if t.shape[0] != c:
            raise ValueError("scale_shift_act: per-channel vectors must be [C]")
    if out is None:
        out = torch.empty_like(x)
    _lib.call("lf_scale_shift_act_f32", x.data_ptr(), out.data_ptr(), n, c, h * w, scale.data_ptr(),
              shift.data_ptr(), 1 if relu else 0, _stream())
    return out


def bn_train_stats(y, gamma, beta, mmean, mvar, stats, momentum=0.99, eps=1e-3):
    """stats: f32 [4,C] rows = mean, invstd, scale, shift (written)."""
    _chk(y, _F32, "bn_train_stats.y", 4)
    n, c, h, w = y.shape
    for t in (gamma, beta, mmean, mvar):
        _chk(t, _F32, "bn_train_stats.param", 1)
        if t.shape[0] != c:
            raise ValueError("bn_train_stats: per-channel vectors must be [C]")
    _chk(stats, _F32, "bn_train_stats.stats", 2)
    if tuple(stats.shape) != (4, c):
        raise ValueError("bn_train_stats.stats: expected [4,C]")
    nbytes = _lib.load().lf_bn_workspace(c)
    ws = _workspace(nbytes, y.device)
    _lib.call("lf_bn_train_stats_f32", y.data_ptr(), n, c, h * w, gamma.data_ptr(), beta.data_ptr(),
              mmean.data_ptr(), mvar.data_ptr(), float(momentum), float(eps), stats[0].data_ptr(),
              stats[1].data_ptr(), stats[2].data_ptr(), stats[3].data_ptr(), ws.data_ptr(),
              ws.numel(), _stream())
    return stats


def bn_infer_scale_shift(gamma, beta, mmean, mvar, stats, eps=1e-3):
    c = gamma.shape[0]
    _lib.call("lf_bn_infer_scale_shift_f32", c, gamma.data_ptr(), beta.data_ptr(), mmean.data_ptr(),
              mvar.data_ptr(), float(eps), stats[2].data_ptr(), stats[3].data_ptr(), _stream())
    return stats


def bn_bwd(g, y, stats, gamma, dgamma, dbeta, relu: bool, alpha_nc=None, add_nc=None, out=None,
           plane_g=None, plane_m=None, tile_sums=None):
    """BatchNorm backward; the ReLU mask (relu=True) is recomputed from y and stats[2:4].
    plane_g ([N,C,2] from block_tail_bwd) / plane_m ([N,C,2] from gap) replace the reduction
    pass over g and y; so do tile_sums (from conv2d_bnbwd, which produced g)."""
    _chk(g, _F32, "bn_bwd.g", 4)
    _chk(y, _F32, "bn_bwd.y", 4)
    if g.shape != y.shape:
        raise ValueError("bn_bwd: g and y must share a shape")
    n, c, h, w = y.shape
    for t in (plane_g, plane_m):
        if t is not None:
            _chk(t, _F32, "bn_bwd.plane sums", 3)
            if tuple(t.shape) != (n, c, 2):
                raise ValueError("bn_bwd: plane sums must be [N,C,2]")
    for t in (alpha_nc, add_nc):
        if t is not None:
            _chk(t, _F32, "bn_bwd.alpha/add", 2)
            if tuple(t.shape) != (n, c):
                raise ValueError("bn_bwd: alpha/add must be [N,C]")
    if out is None:
        out = torch.empty_like(y)
    have = 1 if tile_sums is not None else 0
    if have:   # dgamma / dbeta come from the tiles; only the apply pass runs below
        ws = _bn_bwd_coef("bn_bwd", stats, gamma, dgamma, dbeta, relu, n, c, h * w, y.device, alpha_nc=alpha_nc,
                          add_nc=add_nc, plane_g=plane_g, tile_sums=tile_sums)[1]
    else:
        ws = _workspace(_lib.load().lf_bn_workspace(c), y.device)
    _lib.call("lf_bn_bwd_f32", g.data_ptr(), _ptr(alpha_nc), _ptr(add_nc), y.data_ptr(),
              stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), stats[3].data_ptr(),
              1 if relu else 0, gamma.data_ptr(), out.data_ptr(), dgamma.data_ptr(),
              dbeta.data_ptr(), _ptr(plane_g), _ptr(plane_m), have, n, c, h * w, ws.data_ptr(),
              ws.numel(), _stream())
    return out


def _plane_dtype(t: torch.Tensor, name: str, ndim: int):
    """Checks a plane-kernel tensor stored as fp32 or bf16 and returns its dtype."""
    return _chk(t, _BF16 if t.dtype == _BF16 else _F32, name, ndim).dtype


def gap(x, out=None, scale=None, shift=None, relu: bool = False, mask_sums=None):
    """[N,C,H,W] fp32 or bf16 -> [N,C] fp32 mean of act(x*scale[c]+shift[c]) (plain mean without scale).
    mask_sums [N,C,2] (optional) receives {count of x*scale+shift > 0, sum of x over those}."""
    bf16 = _plane_dtype(x, "gap.x", 4) == _BF16
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty((n, c), dtype=_F32, device=x.device)
    if mask_sums is not None:
        _chk(mask_sums, _F32, "gap.mask_sums", 3)
        if tuple(mask_sums.shape) != (n, c, 2):
            raise ValueError("gap.mask_sums: expected [N,C,2]")
    if bf16:
        _lib.call("lf_gap_stats_bf16", x.data_ptr(), out.data_ptr(), _ptr(mask_sums), n, c, h * w, _ptr(scale),
                  _ptr(shift), 1 if relu else 0, _stream())
    else:
        _lib.call("lf_gap_f32", x.data_ptr(), out.data_ptr(), n * c, h * w, c, _ptr(scale), _ptr(shift),
                  1 if relu else 0, _ptr(mask_sums), _stream())
    return out


def bcast_planes(v, h, w, scale, out=None):
    """out[n,c,:,:] = v[n,c] * scale; out is fp32 (allocated when None) or bf16."""
    _chk(v, _F32, "bcast_planes.v", 2)
    n, c = v.shape
    if out is None:
        out = torch.empty((n, c, h, w), dtype=_F32, device=v.device)
    entry = "lf_bcast_planes_bf16" if _plane_dtype(out, "bcast_planes.out", 4) == _BF16 else "lf_bcast_planes_f32"
    _lib.call(entry, v.data_ptr(), out.data_ptr(), n * c, h * w, float(scale), _stream())
    return out


def cam_maps(feat, w, classes, out=None, peak=None):
    """Class activation maps of the dense head: feat [N,K,h,w] fp32 or bf16 (the last stage's pooled output),
    w [K,C] fp32 (dense.w), classes [N,M] int32 with 1 <= M <= 8 and values in [0, C) ->
    (cam [N,M,h,w] fp32 = sum_k w[k, classes[n,j]] * feat[n,k], peak [N,M] fp32 = max(0, max cam)).
    A class outside [0, C) raises LeafHipError before anything is launched (checked on a host copy)."""
    bf16 = _plane_dtype(feat, "cam_maps.feat", 4) == _BF16
    _chk(w, _F32, "cam_maps.w", 2)
    _chk(classes, torch.int32, "cam_maps.classes", 2)
    n, k, h, wd = feat.shape
    c, m = w.shape[1], classes.shape[1]
    if w.shape[0] != k or classes.shape[0] != n:
        raise ValueError(f"cam_maps: w {tuple(w.shape)} / classes {tuple(classes.shape)} do not fit feat "
                         f"{tuple(feat.shape)}")
    if out is None:
        out = torch.empty((n, m, h, wd), dtype=_F32, device=feat.device)
    if peak is None:
        peak = torch.empty((n, m), dtype=_F32, device=feat.device)
    _chk(out, _F32, "cam_maps.out", 4)
    _chk(peak, _F32, "cam_maps.peak", 2)
    if tuple(out.shape) != (n, m, h, wd) or tuple(peak.shape) != (n, m):
        raise ValueError("cam_maps: out must be [N,M,h,w] and peak [N,M]")
    host = classes.cpu()
    _lib.call("lf_cam_maps", feat.data_ptr(), 1 if bf16 else 0, w.data_ptr(), classes.data_ptr(), host.data_ptr(),
              out.data_ptr(), peak.data_ptr(), n, k, h, wd, c, m, _stream())
    return out, peak


def se_fwd(m, w1, b1, w2, b2, z1, s):
    n, c = m.shape
    cr = w1.shape[1]
    if tuple(w1.shape) != (c, cr) or tuple(w2.shape) != (cr, c) or tuple(z1.shape) != (n, cr) \
            or tuple(s.shape) != (n, c):
        raise ValueError("se_fwd: shape mismatch")
    _lib.call("lf_se_fwd_f32", m.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
              b2.data_ptr(), z1.data_ptr(), s.data_ptr(), n, c, cr, _stream())
    return s


def se_bwd(ds, m, z1, s, w1, w2, dm, dw1, db1, dw2, db2, dm_scale: float = 1.0):
    n, c = m.shape
    cr = w1.shape[1]
    ws = _workspace(_lib.load().lf_se_bwd_workspace(n, c, cr), m.device)
    _lib.call("lf_se_bwd_f32", ds.data_ptr(), m.data_ptr(), z1.data_ptr(), s.data_ptr(),
              w1.data_ptr(), w2.data_ptr(), dm.data_ptr(), dw1.data_ptr(), db1.data_ptr(),
              dw2.data_ptr(), db2.data_ptr(), n, c, cr, float(dm_scale), ws.data_ptr(), ws.numel(),
              _stream())
    return dm


def tail_keeps() -> bool:
    """Whether the fp32 training step keeps y / sc at the tail's recorded positions (block_tail_fwd's y_at / sc_at)
    for block_tail_bwd to read."""
    return not _NO_TAIL_KEEP


def block_tail_fwd(y, a_scale, a_shift, s, sc, sc_scale, sc_shift, sc_relu, drop, route, p, y_at=None, sc_at=None):
    """Add -> ReLU -> SpatialDropout2D -> MaxPool2D(2) on fp32 or bf16 tensors; route: uint8 [N,C,H/2,W/2]
    (written), or None on bf16 tensors when no backward pass follows.  y_at / sc_at (fp32, shaped like p; written):
    the raw y / sc at the position each route byte records, for block_tail_bwd."""
    dt = _plane_dtype(y, "block_tail_fwd.y", 4)
    _chk(sc, dt, "block_tail_fwd.sc", 4)
    _chk(p, dt, "block_tail_fwd.p", 4)
    n, c, h, w = y.shape
    if route is not None:
        _chk(route, torch.uint8, "block_tail_fwd.route", 4)
    if sc.shape != y.shape or tuple(p.shape) != (n, c, h // 2, w // 2) or (route is not None and route.shape != p.shape):
        raise ValueError("block_tail_fwd: shape mismatch")
    if y_at is not None or sc_at is not None:
        _tail_kept("block_tail_fwd", dt, route, p, y_at, sc_at)
        _lib.call("lf_block_tail_fwd_keep_f32", y.data_ptr(), _ptr(a_scale), _ptr(a_shift), _ptr(s), sc.data_ptr(),
                  _ptr(sc_scale), _ptr(sc_shift), 1 if sc_relu else 0, _ptr(drop), _ptr(route), p.data_ptr(),
                  _ptr(y_at), _ptr(sc_at), n, c, h, w, _stream())
        return route, p
    entry = "lf_block_tail_fwd_train_bf16" if dt == _BF16 else "lf_block_tail_fwd_f32"
    _lib.call(entry, y.data_ptr(), _ptr(a_scale), _ptr(a_shift), _ptr(s), sc.data_ptr(), _ptr(sc_scale),
              _ptr(sc_shift), 1 if sc_relu else 0, _ptr(drop), _ptr(route), p.data_ptr(), n, c, h, w, _stream())
    return route, p


def _tail_kept(who: str, dt, route, pooled, y_at, sc_at) -> None:
    """The rules of the tail's kept values: fp32 only, with route bytes, shaped like the pooled tensor."""
    if dt != _F32 or route is None:
        raise ValueError(f"{who}: y_at / sc_at go with fp32 tensors and route bytes")
    for t, nm in ((y_at, "y_at"), (sc_at, "sc_at")):
        if t is not None:
            _chk(t, _F32, f"{who}.{nm}", 4)
            if t.shape != pooled.shape:
                raise ValueError(f"{who}.{nm}: shape mismatch")


def block_tail_bwd(dp, route, y, a_scale, a_shift, drop, dr, ds, plane_sums=None, sc_y=None,
                   sc_sums=None, y_at=None, sc_at=None):
    """y_at / sc_at (block_tail_fwd's): read in place of y / sc_y at the recorded positions; y / sc_y may then be
    None."""
    dt = _plane_dtype(dr, "block_tail_bwd.dr", 4)
    _chk(dp, dt, "block_tail_bwd.dp", 4)
    _chk(route, torch.uint8, "block_tail_bwd.route", 4)
    n, c, h, w = dr.shape
    if tuple(dp.shape) != (n, c, h // 2, w // 2) or route.shape != dp.shape:
        raise ValueError("block_tail_bwd: shape mismatch")
    for t in (plane_sums, sc_sums):
        if t is not None and tuple(t.shape) != (n, c, 2):
            raise ValueError("block_tail_bwd plane sums: expected [N,C,2]")
    if sc_y is not None and sc_y.shape != dr.shape:
        raise ValueError("block_tail_bwd.sc_y: shape mismatch")
    if y_at is not None or sc_at is not None:
        _tail_kept("block_tail_bwd", dt, route, dp, y_at, sc_at)
        _lib.call("lf_block_tail_bwd_kept_f32", dp.data_ptr(), route.data_ptr(), _ptr(y), _ptr(y_at), _ptr(a_scale),
                  _ptr(a_shift), _ptr(drop), dr.data_ptr(), _ptr(ds), _ptr(plane_sums), _ptr(sc_y), _ptr(sc_at),
                  _ptr(sc_sums), n, c, h, w, _stream())
        return dr, ds
    entry = "lf_block_tail_bwd_bf16" if dt == _BF16 else "lf_block_tail_bwd_f32"
    _lib.call(entry, dp.data_ptr(), route.data_ptr(), _ptr(y), _ptr(a_scale), _ptr(a_shift), _ptr(drop),
              dr.data_ptr(), _ptr(ds), _ptr(plane_sums), _ptr(sc_y), _ptr(sc_sums), n, c, h, w, _stream())
    return dr, ds


def head_fwd(feat, w, b, ytrue, probs, loss):
    n, f = feat.shape
    c = w.shape[1]
    _lib.call("lf_head_fwd_f32", feat.data_ptr(), w.data_ptr(), b.data_ptr(), _ptr(ytrue),
              probs.data_ptr(), _ptr(loss), n, f, c, _stream())
    return probs


def head_bwd(feat, w, probs, ytrue, dlogits, dfeat, dw, db, inv_n):
    n, f = feat.shape
    c = w.shape[1]
    _lib.call("lf_head_bwd_f32", feat.data_ptr(), w.data_ptr(), probs.data_ptr(), ytrue.data_ptr(),
              dlogits.data_ptr(), dfeat.data_ptr(), dw.data_ptr(), db.data_ptr(), n, f, c,
              float(inv_n), _stream())


def _head_distill_checks(who: str, feat, w, shaped) -> Tuple[int, int, int]:
    """(n, f, c) of a distillation head launch; `shaped`: name -> (tensor, expected shape), fp32 contiguous all."""
    if feat.dim() != 2 or w.dim() != 2 or w.shape[0] != feat.shape[1]:
        raise ValueError(f"{who}: feat [N,F] and w [F,C] expected, got {tuple(feat.shape)} and {tuple(w.shape)}")
    n, f = feat.shape
    c = w.shape[1]
    dims = {"n": (n,), "nc": (n, c), "nf": (n, f), "fc": (f, c), "c": (c,)}
    for name, (t, shape) in dict(shaped, feat=(feat, "nf"), w=(w, "fc")).items():
        if t is None:
            continue
        if t.dtype != _F32 or not t.is_contiguous() or t.device != feat.device:
            raise ValueError(f"{who}.{name}: a contiguous float32 tensor on {feat.device} expected")
        if tuple(t.shape) != dims[shape]:
            raise ValueError(f"{who}.{name}: expected {dims[shape]}, got {tuple(t.shape)}")
    return n, f, c


def head_distill_fwd(feat, w, b, ytrue, tprobs, temperature: float, alpha: float, probs, soft, loss, kd=None):
    """The head with a teacher (lf_head_distill_fwd_f32): writes probs, soft = p_T - q_T, loss and (optionally) kd."""
    n, f, c = _head_distill_checks("head_distill_fwd", feat, w, {
        "b": (b, "c"), "ytrue": (ytrue, "nc"), "tprobs": (tprobs, "nc"), "probs": (probs, "nc"),
        "soft": (soft, "nc"), "loss": (loss, "n"), "kd": (kd, "n")})
    _lib.call("lf_head_distill_fwd_f32", feat.data_ptr(), w.data_ptr(), b.data_ptr(), ytrue.data_ptr(),
              tprobs.data_ptr(), float(temperature), float(alpha), probs.data_ptr(), soft.data_ptr(),
              loss.data_ptr(), _ptr(kd), n, f, c, _stream())
    return probs


def head_distill_bwd(feat, w, probs, ytrue, soft, temperature: float, alpha: float, dlogits, dfeat, dw, db, inv_n):
    n, f, c = _head_distill_checks("head_distill_bwd", feat, w, {
        "probs": (probs, "nc"), "ytrue": (ytrue, "nc"), "soft": (soft, "nc"), "dlogits": (dlogits, "nc"),
        "dfeat": (dfeat, "nf"), "dw": (dw, "fc"), "db": (db, "c")})
    _lib.call("lf_head_distill_bwd_f32", feat.data_ptr(), w.data_ptr(), probs.data_ptr(), ytrue.data_ptr(),
              soft.data_ptr(), float(temperature), float(alpha), dlogits.data_ptr(), dfeat.data_ptr(),
              dw.data_ptr(), db.data_ptr(), n, f, c, float(inv_n), _stream())


def focal_gamma(who: str, gamma) -> float:
    """The focal exponent as the weighted head takes it: 0, or 1 <= gamma <= 8 (lf_head_focal_fwd_f32 says why)."""
    gamma = float(gamma)
    if not (gamma == 0.0 or 1.0 <= gamma <= 8.0):
        raise ValueError(f"{who}: gamma must be 0 or lie in [1, 8], got {gamma}")
    return gamma


def head_focal_fwd(feat, w, b, ytrue, cw, gamma: float, probs, loss, sw=None):
    """The weighted head (lf_head_focal_fwd_f32): class weights cw [C] (or None) and the focal factor
    (1 - p)^gamma; writes probs, loss and (optionally) sw, the weight s of every sample."""
    n, f, c = _head_distill_checks("head_focal_fwd", feat, w, {
        "b": (b, "c"), "ytrue": (ytrue, "nc"), "cw": (cw, "c"), "probs": (probs, "nc"), "loss": (loss, "n"),
        "sw": (sw, "n")})
    _lib.call("lf_head_focal_fwd_f32", feat.data_ptr(), w.data_ptr(), b.data_ptr(), ytrue.data_ptr(), _ptr(cw),
              focal_gamma("head_focal_fwd", gamma), probs.data_ptr(), loss.data_ptr(), _ptr(sw), n, f, c, _stream())
    return probs


def head_focal_bwd(feat, w, probs, ytrue, cw, gamma: float, dlogits, dfeat, dw, db, inv_n):
    n, f, c = _head_distill_checks("head_focal_bwd", feat, w, {
        "probs": (probs, "nc"), "ytrue": (ytrue, "nc"), "cw": (cw, "c"), "dlogits": (dlogits, "nc"),
        "dfeat": (dfeat, "nf"), "dw": (dw, "fc"), "db": (db, "c")})
    _lib.call("lf_head_focal_bwd_f32", feat.data_ptr(), w.data_ptr(), probs.data_ptr(), ytrue.data_ptr(), _ptr(cw),
              focal_gamma("head_focal_bwd", gamma), dlogits.data_ptr(), dfeat.data_ptr(), dw.data_ptr(),
              db.data_ptr(), n, f, c, float(inv_n), _stream())


def mul(a, b, out):
    if a.shape != b.shape or out.shape != a.shape:
        raise ValueError("mul: shape mismatch")
    _lib.call("lf_mul_f32", a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream())
    return out


def adamw_step(param, grad, m, v, ema, offsets, l2, max_count, lr, step, beta1=0.9, beta2=0.999,
               eps=1e-7, weight_decay=1e-4, clipnorm=0.5, ema_decay=0.999, ema_copy=False,
               norms=None):
    nt = offsets.numel() - 1
    if norms is None:
        norms = torch.empty(nt, dtype=_F32, device=param.device)
    ws = _workspace(_lib.load().lf_adamw_workspace(nt), param.device)
    _lib.call("lf_adamw_step_f32", param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
              _ptr(ema), offsets.data_ptr(), l2.data_ptr(), nt, int(max_count), float(lr),
              float(beta1), float(beta2), float(eps), float(weight_decay), float(clipnorm),
              int(step), float(ema_decay), 1 if ema_copy else 0, norms.data_ptr(), ws.data_ptr(),
              ws.numel(), _stream())
    return norms


def ema_update(ema, w, decay, copy):
    _lib.call("lf_ema_update_f32", ema.data_ptr(), w.data_ptr(), w.numel(), float(decay),
              1 if copy else 0, _stream())
