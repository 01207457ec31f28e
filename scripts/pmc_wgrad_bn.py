"""Run the fused-BatchNorm fp32 weight gradient of the benchmark's eight 3x3 and three 1x1 layers (batch 256), two
launches per layer in model order, for PMC collection (rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, one pass each).
The second launch of a layer is the one to read: the first also raises the kernel's LDS limit."""
import sys
import torch
sys.path.insert(0, ".")
from leaffliction_amd import _lib, nn
dev = torch.device("cuda:0")
n = 256
# cin, cout, size, ksize, alpha/add (the c2 layers' squeeze-excitation gate)
LAYERS = [(32, 32, 224, 3, False), (32, 32, 224, 3, True), (32, 64, 112, 3, False), (64, 64, 112, 3, True),
          (32, 64, 112, 1, False), (64, 128, 56, 3, False), (128, 128, 56, 3, True), (64, 128, 56, 1, False),
          (128, 256, 28, 3, False), (256, 256, 28, 3, True), (128, 256, 28, 1, False)]
lib = _lib.load()
for cin, cout, hw, k, se in LAYERS:
    x = torch.randn(n, cin, hw, hw, device=dev)
    g = torch.randn(n, cout, hw, hw, device=dev)
    y = torch.randn(n, cout, hw, hw, device=dev)
    dyo = torch.empty(n, cout, hw, hw, device=dev)
    coef = torch.randn(5, cout, device=dev)
    al, ad = torch.rand(n, cout, device=dev) + 0.5, torch.randn(n, cout, device=dev) * 0.1
    ws = nn._workspace(lib.lf_conv2d_wgrad_workspace(n, cin, hw, hw, cout, k), dev)
    for _ in range(2):
        _lib.call("lf_conv2d_wgrad_bn_f32", x.data_ptr(), g.data_ptr(), y.data_ptr(), al.data_ptr() if se else None,
                  ad.data_ptr() if se else None, coef.data_ptr(), 1, dyo.data_ptr(), n, cin, hw, hw, cout, k, None,
                  None, 0, ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    del x, g, y, dyo
