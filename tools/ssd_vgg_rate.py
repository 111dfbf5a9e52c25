"""Training images/s of the VGG-DCT SSD300 (`ssd_300DCT`) at B=32 in the arithmetic modes float32 (the default mix),
float32_mfma and float16, with the ResNet50-DCT detectors `ssd_custom` and `deconv` from the same run as the yardstick:

    DJ_AUTOTUNE=1 python tools/ssd_vgg_rate.py --runs 3 --steps 50

Names on the command line select the models (default: ssd_300DCT ssd_custom deconv), --modes a,b,c the modes.  Tiles
are timed at plan time (DJ_AUTOTUNE=1) for geometries the tuning tables do not hold, as for the VGG classifiers in
tools/cls_rate.py.  Per model and mode: --runs blocks of --steps steps, every block and their median; then the share of the
step that is not a GEMM: the step on one stream (side stream off) against the sum of its implicit-GEMM launches timed
one by one on the plan's own buffers."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from jpeg_detection_resnet_ssd_amd import workloads
from jpeg_detection_resnet_ssd_amd.keras import backend as K

B = 32
argv, opts = sys.argv[1:], {"--runs": 1, "--steps": 20, "--modes": "float32,float32_mfma,float16"}
for flag in opts:
    if flag in argv:
        i = argv.index(flag)
        opts[flag] = type(opts[flag])(argv[i + 1])
        del argv[i:i + 2]
runs, n, modes = opts["--runs"], opts["--steps"], opts["--modes"].split(",")
known = ("ssd_300DCT", "ssd_custom", "deconv", "up_sampling")
unknown = [a for a in argv if a not in known]
if unknown:
    sys.exit("unknown model %s: choose among %s" % (unknown, ", ".join(known)))


def timed(fn, reps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


for archi in (argv or ["ssd_300DCT", "ssd_custom", "deconv"]):
    for mode in modes:
        K.set_floatx(mode)
        m, sizes = workloads.build_ssd(archi)
        x, y = workloads.synthetic_batch(archi, sizes, B, fast=True)
        plan = m._plan(B, True, True)
        m._upload(plan, x, y)
        for _ in range(3): m.run_train_step(plan)
        tag = "%-11s %-12s B=%d" % (archi, mode, B)
        rates = []
        for _ in range(runs):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(n): m.run_train_step(plan)
            torch.cuda.synchronize()
            rates.append(B * n / (time.perf_counter() - t0))
            print("%s: %.0f img/s" % (tag, rates[-1]), flush=True)
        med = float(np.median(rates))
        print("%s: median of %d: %.0f img/s = %.1f ms/step, %.1f TFLOP/s algorithmic" % (
            tag, runs, med, 1e3 * B / med, med * workloads.TRAIN_GFLOP_PER_IMAGE[archi] / 1e3), flush=True)
        # everything on one stream, then the GEMMs of the same plan alone
        plan.side_enabled = False
        one_stream = timed(lambda: m.run_train_step(plan), max(3, n // 4))
        gemm = sum(timed(fn, 3) for _, _, fn in plan.conv_calls)
        plan.side_enabled = True
        print("%s: one stream %.2f ms/step, %d GEMM launches one by one %.2f ms, not a GEMM: %.0f %%" % (
            tag, one_stream, len(plan.conv_calls), gemm, 100.0 * (1.0 - gemm / one_stream)), flush=True)
        del m, plan
        torch.cuda.empty_cache()
K.set_floatx("float32")
