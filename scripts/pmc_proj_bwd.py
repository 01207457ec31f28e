"""Run the backward of the benchmark's two fused projection shortcuts (batch 256: 32 -> 64 at 112x112, 64 -> 128 at
56x56), three launches per layer of the fused kernel and of the route it replaces, for PMC collection (rocprofv3 --pmc
FETCH_SIZE / --pmc WRITE_SIZE, one pass each) or a kernel trace.  The last launch of each is the one to read.  Without
a profiler it prints the mean time of the last two launches (HIP events)."""
import sys
import torch
sys.path.insert(0, ".")
from leaffliction_amd import _lib, nn
dev = torch.device("cuda:0")
n = 256
LAYERS = [(32, 64, 112), (64, 128, 56)]
lib = _lib.load()


def timed(fn, reps=3):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return sum(ev[i].elapsed_time(ev[i + 1]) for i in range(1, reps)) / (reps - 1) * 1e3


for cin, cout, hw in LAYERS:
    x = torch.randn(n, cin, hw, hw, device=dev)
    g = torch.randn(n, cout, hw, hw, device=dev)
    y = torch.randn(n, cout, hw, hw, device=dev)
    dyp = torch.empty(n, cout, hw, hw, device=dev)
    dx = torch.empty(n, cin, hw, hw, device=dev)
    w = torch.randn(cin, 1, cout, device=dev) * 0.1
    dw = torch.empty(cin, 1, cout, device=dev)
    coef = torch.randn(5, cout, device=dev)
    assert lib.lf_conv2d_proj_bwd_supported(x.data_ptr(), g.data_ptr(), y.data_ptr(), w.data_ptr(), dx.data_ptr(), n,
                                            cin, hw, hw, cout)
    ws = nn._workspace(max(lib.lf_conv2d_proj_bwd_workspace(n, cin, hw, hw, cout),
                           lib.lf_conv2d_wgrad_workspace(n, cin, hw, hw, cout, 1)), dev)

    def fused():
        _lib.call("lf_conv2d_proj_bwd_f32", x.data_ptr(), g.data_ptr(), y.data_ptr(), coef.data_ptr(), 0, w.data_ptr(),
                  dx.data_ptr(), dw.data_ptr(), n, cin, hw, hw, cout, ws.data_ptr(), ws.numel(), None)

    def pair():
        _lib.call("lf_conv2d_wgrad_bn_f32", x.data_ptr(), g.data_ptr(), y.data_ptr(), None, None, coef.data_ptr(), 0,
                  dyp.data_ptr(), n, cin, hw, hw, cout, 1, None, None, 0, ws.data_ptr(), ws.numel(), None)
        _lib.call("lf_conv2d_wgrad_reduce_f32", ws.data_ptr(), dw.data_ptr(), n, cin, hw, hw, cout, 1, 0.0, None)
        nn.conv2d(dyp, nn.conv2d_dgrad_weights(w, 1), 1, out=dx)

    t_f, t_p = timed(fused), timed(pair)
    gb = 4.0 * n * hw * hw * (2 * cin + 2 * cout) / 1e9
    print(f"{cin}->{cout}@{hw}: fused {t_f:.0f} us ({gb / t_f * 1e3:.2f} TB/s of {gb:.2f} GB), pair {t_p:.0f} us")
    del x, g, y, dyp, dx
