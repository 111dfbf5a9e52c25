"""Achieved bandwidth of the optimizer update kernels: dj_sgd_momentum_update, dj_adam_update (plain and amsgrad),
dj_adadelta_update, dj_rmsprop_update, dj_adagrad_update, dj_adamax_update and dj_nadam_update, each as ONE launch over n elements, for n = the trainable parameters of the deconv SSD300 and of
vgga_dct (as laid out in the flat buffer).  Per launch: bytes moved (every stream read once and written once), microseconds
(the median of 20 samples after warm-up; a sample is --reps launches back to back between two events) and GB/s.

    python tools/optim_rate.py                    # the table
    python tools/optim_rate.py --train-step       # also: one SSD300 training step (deconv, B=32) with SGD and with Adam

All are rules of one kernel (csrc/dj_optim.hip), so none is a yardstick for the others: a change of that kernel is
measured against the build before it, the two libraries alternating in one session (DJ_LIB_PATH selects the library)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from jpeg_detection_resnet_ssd_amd import workloads
from jpeg_detection_resnet_ssd_amd.engine import call
from jpeg_detection_resnet_ssd_amd.keras import backend as K
from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD, Adam, Nadam

SAMPLES, WARMUP = 20, 5


def trainable_count(model):
    """Elements of the flat buffer the optimizer walks: every trainable weight, padded to a multiple of four."""
    return sum((w.size + 3) // 4 * 4 for w in model.weight_specs if w.trainable)


def model_sizes():
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.networks import vgga_dct
    ssd, _ = workloads.build_ssd("deconv", compile_model=False)
    K.clear_session()
    return [("deconv SSD300", trainable_count(ssd)), ("vgga_dct", trainable_count(vgga_dct(1000)))]


def launches(n, dev):
    """name -> (bytes per element, launch closure); l2 and the sum of squares as the l2 segments of a model have them."""
    buf = lambda: torch.zeros(n, dtype=torch.float32, device=dev)
    p = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev) * 0.01
    s1, s2, s3, ssq = buf(), buf(), buf(), torch.zeros(1, device=dev)
    return {
        "dj_sgd_momentum_update": (20, lambda: call("dj_sgd_momentum_update", p, g, s1, n, 1e-3, 0.9, 0, 5e-4, 1.0, ssq)),
        "dj_adam_update": (28, lambda: call("dj_adam_update", p, g, s1, s2, None, n, 1e-3, 0.9, 0.999, 1e-7, 5e-4, 1.0, ssq)),
        "dj_adam_update amsgrad": (36, lambda: call("dj_adam_update", p, g, s1, s2, s3, n, 1e-3, 0.9, 0.999, 1e-7, 5e-4, 1.0,
                                                    ssq)),
        "dj_adadelta_update": (28, lambda: call("dj_adadelta_update", p, g, s1, s2, n, 1.0, 0.95, 0.05, 1e-7, 5e-4, 1.0, ssq)),
        "dj_rmsprop_update": (20, lambda: call("dj_rmsprop_update", p, g, s1, n, 1e-3, 0.9, 1e-7, 5e-4, 1.0, ssq)),
        "dj_adagrad_update": (20, lambda: call("dj_adagrad_update", p, g, s1, n, 1e-2, 1e-7, 5e-4, 1.0, ssq)),
        "dj_adamax_update": (28, lambda: call("dj_adamax_update", p, g, s1, s2, n, 2e-2, 0.9, 0.999, 1e-7, 5e-4, 1.0, ssq)),
        "dj_nadam_update": (28, lambda: call("dj_nadam_update", p, g, s1, s2, n, 2e-3, 0.9, 0.999, 1e-7, *Nadam().step_scalars(),
                                             5e-4, 1.0, ssq)),
    }


def median_us(fn, reps):
    for _ in range(WARMUP * reps):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(SAMPLES):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def train_step_ms(optimizer, batch, steps):
    model, sizes = workloads.build_ssd("deconv", compile_model=False)
    from jpeg_detection_resnet_ssd_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    model.compile(optimizer=optimizer, loss=SSDLoss(neg_pos_ratio=3, alpha=1.0).compute_loss)
    x, y = workloads.synthetic_batch("deconv", sizes, batch, fast=True)
    plan = model._plan(batch, True, True)
    model._upload(plan, x, y)
    for _ in range(5):
        model.run_train_step(plan)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.run_train_step(plan)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    del model, plan
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="launches back to back per sample")
    ap.add_argument("--train-step", action="store_true", help="also time SSD300 (deconv) training steps with SGD and Adam")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing here can be measured without one")
    dev = torch.device("cuda:0")
    print("| n | launch | bytes | us (median of %d; min .. max) | GB/s |" % SAMPLES)
    print("|---|---|---|---|---|")
    for what, n in model_sizes():
        for name, (bpe, fn) in launches(n, dev).items():
            us, lo, hi = median_us(fn, args.reps)
            print("| %s (%d) | %s | %d | %.1f (%.1f .. %.1f) | %.0f |" % (what, n, name, bpe * n, us, lo, hi, bpe * n / us / 1e3),
                  flush=True)
        torch.cuda.empty_cache()
    if args.train_step:
        for name, opt in (("SGD(0.001, 0.9)", SGD(lr=0.001, momentum=0.9)), ("Adam(0.001)", Adam(lr=0.001)),
                          ("SGD(0.001, 0.9) again", SGD(lr=0.001, momentum=0.9))):
            print("deconv SSD300 %s B=%d %s: %.2f ms/step" % (K.floatx(), args.batch, name,
                                                             train_step_ms(opt, args.batch, args.steps)), flush=True)


if __name__ == "__main__":
    main()
