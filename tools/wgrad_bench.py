"""Times the fp32 weight gradient (cn_conv2d_bwd_weight_f32, contraction + slice sum) of a few layer shapes of the default
step, 3 x 3 or 1 x 1 (padding k // 2):
python tools/wgrad_bench.py [k]                  (B Cin H W Cout rows from the list below)
python tools/wgrad_bench.py B Cin H W Cout [k]   (one shape)
CN_LIB_PATH selects another build of the library for an A/B."""
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from cultionet_amd import _lib  # noqa: E402

shapes = {3: [(8, 128, 100, 100, 128), (8, 32, 100, 100, 32), (8, 160, 100, 100, 128), (8, 64, 50, 50, 64), (8, 128, 26, 26, 128)],
          # the 1 x 1 layers of the default step (tools/layers_iso.py), largest first; 25 x 25 goes through the aligned copies
          1: [(8, 480, 100, 100, 128), (8, 128, 100, 100, 384), (8, 576, 50, 50, 128), (8, 128, 100, 100, 128),
              (8, 1152, 25, 25, 128), (8, 128, 50, 50, 384), (8, 256, 13, 13, 128), (8, 36, 100, 100, 30)]}
args = [int(v) for v in sys.argv[1:]]
k = args[-1] if len(args) in (1, 6) else 3
assert k in shapes, "kernel size 1 or 3"
rows = [tuple(args[:5])] if len(args) >= 5 else shapes[k]
dev = torch.device("cuda:0")
s = torch.cuda.current_stream().cuda_stream
for B, Cin, H, W, Cout in rows:
    x = torch.randn(B, Cin, H, W, device=dev)
    dy = torch.randn(B, Cout, H, W, device=dev)
    nws = B * (Cout * (H * (W + 1) + 3) + Cin * (H * W + 3)) + (1 << 24)
    ws = torch.empty(nws, device=dev)
    dw = torch.zeros(Cout, Cin, k, k, device=dev)

    def run():
        _lib.call("cn_conv2d_bwd_weight_f32", x.data_ptr(), Cin * H * W, dy.data_ptr(), Cout * H * W, dw.data_ptr(), B, Cin,
                  H, W, Cout, k, k, 1, k // 2, 1, ws.data_ptr(), nws, s)

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    n = 200
    t0 = time.perf_counter()
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    fl = 2.0 * B * H * W * Cin * Cout * k * k
    dw.zero_()
    run()
    ref = torch.nn.grad.conv2d_weight(x, dw.shape, dy, padding=k // 2)
    err = float((dw - ref).abs().max() / ref.abs().max())
    print(f"B={B} {Cin}->{Cout} {H}x{W} k{k}: {dt * 1e6:7.1f} us  {fl / dt / 1e12:6.1f} TFLOP/s ({fl / dt / 157.3e12:.3f} of the f32 peak)  rel err {err:.1e}")
