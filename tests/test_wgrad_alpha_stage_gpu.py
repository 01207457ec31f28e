"""The per-image alpha / add of the fused BatchNorm-backward weight gradient (wgrad3_kernel), which the kernel keeps in
a two-slot LDS table that it refills when its walk over the items enters a new image; and the BatchNorm-backward
sums entries, which form the five apply coefficients in the kernel that forms the sums.

Rows: one per wgrad3_kernel instantiation, found through lf_conv2d_wgrad_plan so that the variant is the wanted
one, staging is the vector path, a split walks 3 items, an image's item count is no multiple of that (so a new image
opens at the first, the middle and the last item of some split) and n >= 5 (both table slots are reused).  The split
arithmetic restated here is plan_wgrad's: 512 workgroups over the channel blocks, the same item count per split.

alpha is a power of two per (image, channel), so g * alpha is exact and the host's fmaf below (one product and one
sum in float64, rounded to fp32) is the device's fmaf bit for bit: the sum of two fp32 values either is exact in
float64 or lies within 2^-29 of the larger one, far from any fp32 tie.

Per case:
 (i)   dy_out and dW are byte-equal to the same entry given g' = fmaf(g, alpha, add) and no alpha / add (bn_dy1 with
       alpha 1, add 0 leaves g' as it is), so one stale or misplaced table entry is a bit difference;
 (ii)  the result differs, image by image, from the one with every image sharing image 0's alpha / add where the
       image's own differ: a table that is never refilled would not pass (i) by accident of the data;
 (iii) dW holds test_wgrad_winograd_gpu's float64 bound, TAU_WG times the sum of the absolute terms, over the
       kernel's own dY.
"""
import ctypes

import pytest
import torch

from test_wgrad_winograd_gpu import D, TAU_WG, WG_TILE, _wild, fmaf, wgrad_ref

pytestmark = pytest.mark.gpu

# block of input / output channels per variant (kWgVariants)
WG_BLOCK = {0: (32, 32), 1: (32, 64), 2: (64, 64), 3: (64, 64)}

# n, cin, cout, h, w, variant
ROWS = [
    (33, 40, 40, 14, 64, 0),    # <32,4,1,1,4>, Cin / Cout = 32 + 8
    (11, 40, 40, 56, 112, 1),   # <16,8,1,2,2>: the dY tile in two halves
    (21, 40, 40, 28, 112, 2),   # <16,4,2,2,1>
    (9, 40, 40, 58, 112, 3),    # <28,2,2,2,1>
]
# prologue, add
MODES = [(False, False), (False, True), (True, False), (True, True)]


def _lib():
    from leaffliction_amd import _lib as L
    return L


def split_walk(n, cin, cout, h, w, variant):
    """(items per image, items per split) of plan_wgrad for a 3x3 layer."""
    tw, th = WG_TILE[variant]
    ci_t, co_t = WG_BLOCK[variant]
    tiles = (w // tw) * ((h + th - 1) // th)
    items = n * tiles
    splits = min(max(512 // (((cin + ci_t - 1) // ci_t) * ((cout + co_t - 1) // co_t)), 1), items)
    return tiles, (items + splits - 1) // splits


def test_rows_reach_their_plans():
    lib = _lib().load()
    for n, cin, cout, h, w, variant in ROWS:
        out = (ctypes.c_int * 4)()
        assert lib.lf_conv2d_wgrad_plan(n, cin, h, w, cout, 3, out) == 0
        assert (out[0], out[1], out[3]) == (variant, 3, 1), (n, cin, cout, h, w, tuple(out))
        assert w % WG_TILE[variant][0] == 0 and w % 4 == 0 and n >= 5
        tiles, ips = split_walk(n, cin, cout, h, w, variant)
        assert ips >= 3 and tiles % ips != 0
        opens = {(k * tiles) % ips for k in range(1, n)}   # where in its split an image's first item stands
        assert 0 in opens and ips - 1 in opens and any(0 < r < ips - 1 for r in opens), (tiles, ips, opens)
    assert {r[5] for r in ROWS} == {0, 1, 2, 3}


def call_wgrad_bn(cuda, t, g, al, ad):
    """lf_conv2d_wgrad_bn_f32 + reduce on device tensors: (dy_out, dw)."""
    from leaffliction_amd import nn
    n, cin, h, w = t["x"].shape
    cout = g.shape[1]
    lib = _lib().load()
    p = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    ws = nn._workspace(lib.lf_conv2d_wgrad_workspace(n, cin, h, w, cout, 3), cuda)
    dyo = torch.empty(n, cout, h, w, device=cuda)
    dw = torch.empty(cin, 9, cout, device=cuda)
    _lib().call("lf_conv2d_wgrad_bn_f32", t["x"].data_ptr(), g.data_ptr(), t["y"].data_ptr(), p(al), p(ad),
                t["coef"].data_ptr(), 1, dyo.data_ptr(), n, cin, h, w, cout, 3, p(t["sc"]), p(t["sh"]),
                1 if t["sc"] is not None else 0, ws.data_ptr(), ws.numel(), None)
    _lib().call("lf_conv2d_wgrad_reduce_f32", ws.data_ptr(), dw.data_ptr(), n, cin, h, w, cout, 3, 0.0, None)
    torch.cuda.synchronize()
    return dyo.cpu(), dw.cpu()


CASES = [pytest.param(*r, m, id=f"v{r[5]}-{'pro' if m[0] else 'plain'}-{'alpha_add' if m[1] else 'alpha'}")
         for r in ROWS for m in MODES]


@pytest.mark.parametrize("n,cin,cout,h,w,variant,mode", CASES)
def test_alpha_table(cuda, n, cin, cout, h, w, variant, mode):
    pro, with_add = mode
    assert _lib().load().lf_conv2d_wgrad_bn_supported(n, cin, h, w, cout, 3)
    gen = torch.Generator().manual_seed(n * 131 + cin * 7 + cout + h + w + 2 * pro + with_add)
    x, up = _wild((n, cin, h, w), gen), _wild((n, cout, h, w), gen)
    yb = torch.randn(n, cout, h, w, generator=gen) * 1.3 + 0.2
    coef = torch.randn(5, cout, generator=gen) * 0.5
    coef[2] = coef[2].abs() + 0.5
    sc, sh = torch.rand(cin, generator=gen) + 0.5, torch.randn(cin, generator=gen) * 0.3
    # alpha = 2^(e[n] + f[c]): consecutive images differ by a power of two, image 3 repeats image 0's
    e = (torch.arange(n) % 3 - 1).view(n, 1).float()
    f = torch.randint(-1, 2, (1, cout), generator=gen).float()
    al = torch.exp2(e + f)
    ad = torch.randn(n, cout, generator=gen) * 0.1 * (e + 2) if with_add else None
    d = lambda v: None if v is None else v.to(cuda)  # noqa: E731
    t = dict(x=d(x), y=d(yb), coef=d(coef), sc=d(sc) if pro else None, sh=d(sh) if pro else None)

    dyo, dw = call_wgrad_bn(cuda, t, d(up), d(al), d(ad))

    # (i) the same entry on g' formed by the host, no table
    zero = torch.zeros(n, cout)
    gp = fmaf(up, al.view(n, cout, 1, 1), (ad if with_add else zero).view(n, cout, 1, 1))
    dyo_h, dw_h = call_wgrad_bn(cuda, t, d(gp), None, None)
    bad = (dyo.view(torch.int32) != dyo_h.view(torch.int32)).flatten(1).any(1)
    assert not bool(bad.any()), f"dy_out differs from the host-formed g' in images {bad.nonzero().flatten().tolist()}"
    assert torch.equal(dw.view(torch.int32), dw_h.view(torch.int32)), "dW differs from the host-formed g'"

    # (ii) every image on image 0's alpha / add
    al0 = al[:1].expand(n, cout).contiguous()
    ad0 = ad[:1].expand(n, cout).contiguous() if with_add else None
    dyo_s, dw_s = call_wgrad_bn(cuda, t, d(up), d(al0), d(ad0))
    for img in range(n):
        same = torch.equal(al[img], al[0]) and (not with_add or torch.equal(ad[img], ad[0]))
        assert torch.equal(dyo[img], dyo_s[img]) == same, f"image {img}: own alpha / add against image 0's"
    assert not torch.equal(dw, dw_s)

    # (iii) float64 bound over the kernel's own dY
    a = torch.relu(fmaf(x, sc.view(1, -1, 1, 1), sh.view(1, -1, 1, 1))) if pro else x
    dy = dyo.to(D)
    err = (dw.to(D) - wgrad_ref(a, dy)).abs()
    lim = TAU_WG * wgrad_ref(a.abs(), dy.abs()) + 1e-30
    assert bool((err <= lim).all()), f"worst |err| / bound {float((err / lim).max()):.3g}"


def _bn_inputs(cuda, n, c, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    stats = torch.stack([r(c) * 0.5, torch.rand(c, generator=gen) + 0.5, r(c), r(c)]).to(cuda)
    return gen, r, stats, (torch.rand(c, generator=gen) + 0.5).to(cuda)


def _twice(c, cuda, call):
    """Two calls into the same dgamma / dbeta / coef buffers (pre-filled differently): the bytes of each."""
    dg, db, coef = (torch.empty(c, device=cuda), torch.empty(c, device=cuda), torch.empty(5, c, device=cuda))
    res = []
    for fill in (3.0, -7.0):
        for buf in (dg, db, coef):
            buf.fill_(fill)
        call(dg, db, coef)
        torch.cuda.synchronize()
        res.append(torch.cat([dg, db, coef.flatten()]).cpu().view(torch.int32))
    return res


@pytest.mark.parametrize("c", [33, 256])
def test_bn_bwd_sums_tiles_repeats(cuda, c):
    """lf_bn_bwd_sums_tiles_f32 (sums, dgamma / dbeta and the coefficients in one finalize kernel): a second call into
    the same buffers gives the first call's bytes; c = 33 is a ragged, 256 a full grid of per-channel threads."""
    from leaffliction_amd import _lib, nn
    n, hw, tiles = 3, 64, 3
    gen, r, st, gam = _bn_inputs(cuda, n, c, 100 + c)
    part = (r(c, tiles, 2) * 4).to(cuda)
    ws = nn._workspace(_lib.load().lf_bn_workspace(c), cuda)

    def call(dg, db, coef):
        _lib.call("lf_bn_bwd_sums_tiles_f32", part.data_ptr(), tiles, st[0].data_ptr(), st[1].data_ptr(),
                  st[2].data_ptr(), st[3].data_ptr(), gam.data_ptr(), dg.data_ptr(), db.data_ptr(), coef.data_ptr(),
                  n, c, hw, ws.data_ptr(), ws.numel(), None)

    first, second = _twice(c, cuda, call)
    assert torch.equal(first, second)
    assert bool(torch.isfinite(first.view(torch.float32)).all())


@pytest.mark.parametrize("c", [33, 256])
def test_bn_bwd_sums_planes_repeats(cuda, c):
    """lf_bn_bwd_sums_f32 on per-plane sums (bn_bwd_planes_kernel forms the coefficients too): the same."""
    from leaffliction_amd import _lib, nn
    n, hw = 3, 64
    gen, r, st, gam = _bn_inputs(cuda, n, c, 200 + c)
    pg, pm = (r(n, c, 2) * 4).to(cuda), (torch.rand(n, c, 2, generator=gen) * hw).to(cuda)
    al, ad = (torch.rand(n, c, generator=gen) + 0.5).to(cuda), (r(n, c) * 0.1).to(cuda)
    ws = nn._workspace(_lib.load().lf_bn_workspace(c), cuda)

    def call(dg, db, coef):
        _lib.call("lf_bn_bwd_sums_f32", None, al.data_ptr(), ad.data_ptr(), None, st[0].data_ptr(), st[1].data_ptr(),
                  st[2].data_ptr(), st[3].data_ptr(), 1, gam.data_ptr(), dg.data_ptr(), db.data_ptr(),
                  coef.data_ptr(), pg.data_ptr(), pm.data_ptr(), n, c, hw, ws.data_ptr(), ws.numel(), None)

    first, second = _twice(c, cuda, call)
    assert torch.equal(first, second)
    assert bool(torch.isfinite(first.view(torch.float32)).all())
