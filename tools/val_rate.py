"""Time of one validation sweep as fit_generator runs it: the deconv classifier at batch 64 and SSD300 deconv at batch 32,
50 batches each on prepared synthetic batches (host batch production is not what is measured), median of 5 sweeps, each
between two device synchronisations, after a warm-up sweep.

    python tools/val_rate.py [--steps 50] [--reps 5]

With the device sweep (Model.evaluate_generator's accumulator) a sweep is forward + dj_eval_accumulate per batch and one
download at its end; on a tree without it the same loop is what fit_generator did there, test_on_batch per batch (a loss
download and the penalty's reductions every batch) -- the tool runs unchanged on both, for before / after figures."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from jpeg_detection_resnet_ssd_amd import workloads  # noqa: E402
from jpeg_detection_resnet_ssd_amd.keras import backend as K  # noqa: E402
from jpeg_detection_resnet_ssd_amd.keras import models  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument("--steps", type=int, default=50)
parser.add_argument("--reps", type=int, default=5)
args = parser.parse_args()
assert torch.cuda.is_available(), "val_rate.py needs an MI355X"
DEVICE_SWEEP = hasattr(models, "_EvalSweep")


def sweep(model, batches, steps):
    """-> the logs a validation sweep of `steps` batches adds: what fit_generator does after an epoch."""
    if DEVICE_SWEEP:
        s = models._EvalSweep(model, size_weighted=False)
        for i in range(steps):
            s.add(*batches[i % len(batches)])
        return s.finish()
    total = 0.0
    for i in range(steps):
        total += model.test_on_batch(*batches[i % len(batches)])
    return {"loss": total / steps}


def measure(name, model, batches, batch_size):
    logs = sweep(model, batches, args.steps)        # warm-up: plan, tuning, code objects
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        logs = sweep(model, batches, args.steps)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    print("%-28s %s sweep of %d x %d: median %.1f ms (min %.1f, max %.1f; %.2f ms / batch, %.0f img/s)  %s"
          % (name, "device" if DEVICE_SWEEP else "test_on_batch", args.steps, batch_size, 1e3 * med, 1e3 * min(times),
             1e3 * max(times), 1e3 * med / args.steps, batch_size * args.steps / med,
             " ".join("%s=%.6g" % kv for kv in logs.items())), flush=True)


spec = importlib.util.spec_from_file_location("cfg_resnet", os.path.join(ROOT, "config", "resnet", "config_file.py"))
cfg_mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cfg_mod)
K.clear_session()
cfg = cfg_mod.TrainingConfiguration(deconv=True, archi="deconv", load_pretrained_weights=False)
classifier = cfg.network
classifier.compile(loss=cfg.loss, optimizer=cfg.optimizer, metrics=cfg.metrics)
gen = cfg_mod.SyntheticDCTClassificationGenerator(64, True, cfg.num_classes, n_batches=4, seed=999983)
measure("classifier deconv, batch 64", classifier, [gen[i] for i in range(len(gen))], 64)
del classifier, cfg
torch.cuda.empty_cache()

ssd, sizes = workloads.build_ssd("deconv")
batches = [workloads.synthetic_batch("deconv", sizes, 32, seed=500 + i, fast=True) for i in range(4)]
batches = [(x, np.ascontiguousarray(y, dtype=np.float32)) for x, y in batches]
measure("SSD300 deconv, batch 32", ssd, batches, 32)
