"""Cost of turning one batch of decoded images (64 images of mixed sizes around 375x500) into the classifier's DCT input
tensors at 224x224, host path vs device path:

  (a) host:   PIL resize + crop + flip on 16 threads, data/jpeg_dct.py:emit_dct_inputs (PIL encode, in-tree entropy
              decoder on 16 threads), float32 upload
  (b) device: DeviceImagePrep: one upload of descriptors + taps + pixels from pinned memory, dj_image_prep, dj_rgb_to_dct
  (c) the two kernels alone, by device events, and their bytes moved over that time
  (d) Model.fit_generator img/s of the batch-64 deconv classifier fed by a generator that emits the same decoded
      batches through (a) or through (b)
  (e) the photometric stage (saturation, brightness, contrast, lighting, each drawn with probability 1/2 per image in a
      shuffled order, as the generators do): the device path with dj_photometric between the two kernels, the kernel
      alone by events, and the four numpy callables on the 64 prepared images on 16 threads
  (f) device decode: the same batch as JPEG files (quality 90; the other rows work on Pillow's pixels of these files).
      Pillow's decode in one thread, which is what (b) leaves in the generator; in its place the headers
      (`CoefficientImage`), `BatchPlan.fill` with the coefficient read on 16 threads and on 1, the upload of the larger
      blob, dj_jpeg_pixels alone and in front of dj_image_prep by events, and the whole `emit_into`; outputs asserted
      equal to (b)'s.  No target: the yardstick is row (b) of the same run

    python tools/prep_rate.py [--reps 20] [--fit-steps 40] [--no-fit]

Medians over `reps` after warm-up; every timed window ends in a device synchronise.  (a), (f) and the host half of (d)
need PIL; without it they are reported as not measured.  Prints one JSON line at the end."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from jpeg_detection_resnet_ssd_amd import kernels
from jpeg_detection_resnet_ssd_amd.data import image_prep, jpeg_dct, photometric

HBM_MEASURED_GBS = 6290.0     # float4 copy on MI355X (tools/input_rate.py)
T = 224


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def event_ms(fn, reps, setup=None):
    """`setup` runs before every repetition, ahead of the first event: its time is not counted."""
    for _ in range(5):
        if setup is not None:
            setup()
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if setup is not None:
            setup()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def make_batch(rng, n):
    """Smooth content plus noise, landscape and portrait, sides within +-15 % of 375 x 500; draws as the generators make."""
    images, params = [], []
    for i in range(n):
        h, w = int(375 * rng.uniform(0.85, 1.15)), int(500 * rng.uniform(0.85, 1.15))
        if i % 3 == 2:
            h, w = w, h
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + 100 * np.sin(xx / (11.0 + c + i % 7) + c) * np.cos(yy / (8.0 + 2 * c)) for c in range(3)], axis=-1)
        images.append(np.clip(img + rng.normal(0, 15, img.shape), 0, 255).astype(np.uint8))
        params.append((True, int(rng.integers(0, image_prep.max_offset(h, w, T) + 1)), bool(rng.random() > 0.5)))
    return images, params


def make_ops(rng, n):
    """Per image: the four operations in a shuffled order, each taken with probability 1/2, parameters as the callables
    draw them."""
    ops = []
    for _ in range(n):
        lst = []
        for code in rng.permutation([photometric.LIGHTING, photometric.CONTRAST, photometric.BRIGHTNESS, photometric.SATURATION]):
            if rng.random() > 0.5:
                lst.append((int(code), tuple(rng.standard_normal(3) * 0.5) if code == photometric.LIGHTING
                            else (0.5 + rng.random(),)))
        ops.append(lst)
    return ops


def as_files(images):
    """-> (the images saved as JPEG at quality 90, Pillow's pixels of those files)."""
    import io

    from PIL import Image
    files, decoded = [], []
    for img in images:
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=90)
        files.append(buf.getvalue())
        decoded.append(pillow_decode(files[-1]))
    return files, decoded


def pillow_decode(data):
    import io

    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def decode_rows(res, files, images, params, bufs, want, dev, reps):
    """Row (f).  `want`: the tensors (b) wrote for the same batch."""
    from jpeg_detection_resnet_ssd_amd.data.jpeg_pixels import CoefficientImage
    res["pillow_decode_1_thread_ms"] = median_ms(lambda: [pillow_decode(f) for f in files], max(5, reps // 2))
    res["decode_headers_ms"] = median_ms(lambda: [CoefficientImage(f) for f in files], reps)
    items = [CoefficientImage(f) for f in files]
    res["files_MB"] = sum(len(f) for f in files) / 1e6
    preps = {n: image_prep.DeviceImagePrep(target_length=T, deconv=True, n_threads=n) for n in (16, 1)}
    pending = preps[16](items, params)
    plan = pending.plan
    assert plan.decode_items == list(range(len(files))), "every file of the batch must travel as coefficients"
    staging = torch.empty(plan.nbytes, dtype=torch.uint8).pin_memory()
    host = staging.numpy()
    for n in (16, 1):
        res["decode_fill_%d_threads_ms" % n] = median_ms(lambda: plan.fill(host, items, n), reps)
        res["device_decode_%d_threads_ms" % n] = median_ms(lambda: preps[n](items, params).emit_into(bufs), reps)
    res["device_decode_emit_only_ms"] = median_ms(lambda: pending.emit_into(bufs), reps)
    torch.cuda.synchronize()
    res["device_decode_equals_device_prep"] = all(torch.equal(a, b) for a, b in zip(want, bufs))
    assert res["device_decode_equals_device_prep"], "device decode and device prep disagree"
    plain = image_prep.BatchPlan([im.shape[:2] for im in images], params, T)
    plain_staging = np.empty(plain.nbytes, dtype=np.uint8)
    res["prep_fill_ms"] = median_ms(lambda: plain.fill(plain_staging, images), reps)      # the pixel copy (b) makes instead
    res["decode_upload_MB"] = plan.nbytes / 1e6
    res["decode_upload_pinned_ms"] = median_ms(lambda: staging.to(dev, non_blocking=True), reps)
    blob = staging.to(dev)
    pixels = torch.empty(plan.out_shape, dtype=torch.uint8, device=dev)
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=dev)
    res["jpeg_pixels_ms"] = event_ms(lambda: plan.launch_decode(host, blob, scratch), max(50, reps))
    res["jpeg_pixels_image_prep_ms"] = event_ms(lambda: plan.launch(host, blob, pixels, scratch), max(50, reps))
    res["decode_plan_ms"] = median_ms(lambda: preps[16](items, params), reps)
    # one batch from files to input tensors: what the generator does (decode or headers, plan) plus the emission
    res["files_to_tensors_ms"] = {"device_prep": res["pillow_decode_1_thread_ms"][0] + res["device_ms"][0],
                                  "device_decode": res["decode_headers_ms"][0] + res["device_decode_16_threads_ms"][0]}


def pil_prep(img, scale, offset, flip):
    from PIL import Image
    im = Image.fromarray(img)
    ratio = T / min(im.size)
    width, height = im.size
    im = im.resize((int(round(width * ratio)), int(round(height * ratio))))
    im = im.crop((offset, 0, T + offset, T)) if im.size[0] > im.size[1] else im.crop((0, offset, T, T + offset))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fit-steps", type=int, default=40)
    ap.add_argument("--no-fit", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prep_rate.py measures on the GPU"
    dev = torch.device("cuda:0")
    B = 64
    rng = np.random.default_rng(0)
    batches = [make_batch(rng, B) for _ in range(2)]
    try:
        import PIL
        have_pil = PIL.__version__
    except ImportError:
        have_pil = False
    files = None
    if have_pil:          # every row works on the pixels of the JPEG files row (f) sends up undecoded
        files, decoded = as_files(batches[0][0])
        batches[0] = (decoded, batches[0][1])
    images, params = batches[0]
    res = {"batch": B, "target": T, "reps": args.reps, "pil": have_pil,
           "source_MB": sum(im.nbytes for im in images) / 1e6}
    shapes = jpeg_dct.input_shapes(B, T, T, deconv=True)
    bufs = [torch.empty(s, device=dev) for s in shapes]
    pool = ThreadPoolExecutor(16)

    def host_pixels(batch):
        return np.stack(list(pool.map(lambda a: pil_prep(a[0], *a[1]), zip(*batch))))

    # (a) host path, and its resize + crop + flip part alone
    if have_pil:
        def host_path():
            for buf, arr in zip(bufs, jpeg_dct.emit_dct_inputs(host_pixels(batches[0]), deconv=True, n_threads=16)):
                buf.copy_(torch.from_numpy(arr), non_blocking=True)
        res["host_ms"] = median_ms(host_path, max(5, args.reps // 2))
        res["host_pil_prep_ms"] = median_ms(lambda: host_pixels(batches[0]), max(5, args.reps // 2))
        want = [b.clone() for b in bufs]
    # (b) device path: the pending batch is made (descriptors, taps) and emitted
    prep = image_prep.DeviceImagePrep(target_length=T, deconv=True)
    res["device_ms"] = median_ms(lambda: prep(images, params).emit_into(bufs), args.reps)
    pending = prep(images, params)
    res["device_emit_only_ms"] = median_ms(lambda: pending.emit_into(bufs), args.reps)
    res["device_plan_ms"] = median_ms(lambda: prep(images, params), args.reps)
    if have_pil:
        res["device_equals_host"] = all(torch.equal(a, b) for a, b in zip(want, bufs))
        res["host_over_device"] = res["host_ms"][0] / res["device_ms"][0]
    # (f) device decode, next to (b)
    if have_pil:
        torch.cuda.synchronize()
        decode_rows(res, files, images, params, bufs, [b.clone() for b in bufs], dev, args.reps)
    else:
        res["device_decode_16_threads_ms"] = "not measured (no PIL)"
    # (c) the two kernels alone, by events
    plan = pending.plan
    staging = torch.empty(plan.nbytes, dtype=torch.uint8).pin_memory()
    plan.fill(staging.numpy(), images)
    res["upload_pinned_ms"] = median_ms(lambda: staging.to(dev, non_blocking=True), args.reps)
    res["upload_MB"] = plan.nbytes / 1e6
    blob = staging.to(dev)
    pixels = torch.empty((B, T, T, 3), dtype=torch.uint8, device=dev)
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=dev)
    host = staging.numpy()
    reps = max(50, args.reps)
    prep_ms = event_ms(lambda: plan.launch(host, blob, pixels, scratch), reps)
    outs = tuple(bufs)
    dct_ms = event_ms(lambda: kernels.rgb_to_dct(pixels, prep.tables, outs), reps)
    d = plan.desc
    rows = d["n_rows"].astype(np.int64)
    prep_bytes = int((rows * d["src_stride"]).sum() + 2 * (rows * 3 * T).sum() + B * T * T * 3 + plan.pool.nbytes)
    dct_bytes = B * T * T * 3 + sum(4 * int(np.prod(s)) for s in shapes)
    res["image_prep_ms"], res["image_prep_bytes"], res["image_prep_GBs"] = prep_ms, prep_bytes, prep_bytes / prep_ms[0] / 1e6
    res["rgb_to_dct_ms"], res["rgb_to_dct_bytes"], res["rgb_to_dct_GBs"] = dct_ms, dct_bytes, dct_bytes / dct_ms[0] / 1e6
    res["kernels_share_of_measured_hbm"] = (prep_bytes + dct_bytes) / (prep_ms[0] + dct_ms[0]) / 1e6 / HBM_MEASURED_GBS
    # (e) the photometric stage
    ops = make_ops(rng, B)
    res["photometric_ops_per_image"] = float(np.mean([len(o) for o in ops]))
    res["device_photometric_ms"] = median_ms(lambda: prep(images, params, ops).emit_into(bufs), args.reps)
    with_ops = prep(images, params, ops)
    res["device_photometric_emit_only_ms"] = median_ms(lambda: with_ops.emit_into(bufs), args.reps)
    ops_host = with_ops.plan.ops
    ops_dev = torch.from_numpy(ops_host.view(np.uint8).reshape(-1).copy()).to(dev)
    plan.launch(host, blob, pixels, scratch)
    prepared_dev = pixels.clone()

    def restore():          # the kernel works in place: every repetition starts from the prepared batch again
        pixels.copy_(prepared_dev)
    res["photometric_ms"] = event_ms(lambda: kernels.photometric(pixels, ops_dev, ops_host), reps, setup=restore)
    all_four = photometric.pack_ops([[(c, (0.1, 0.2, -0.1) if c == photometric.LIGHTING else (0.9,)) for c in (4, 3, 2, 1)]] * B)
    all_dev = torch.from_numpy(all_four.view(np.uint8).reshape(-1).copy()).to(dev)
    res["photometric_all_four_ms"] = event_ms(lambda: kernels.photometric(pixels, all_dev, all_four), reps, setup=restore)
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import brightness, contrast, lighting, saturation
    by_code = {photometric.SATURATION: saturation, photometric.BRIGHTNESS: brightness, photometric.CONTRAST: contrast,
               photometric.LIGHTING: lighting}
    prepared = prepared_dev.cpu().numpy()

    def callables(a):
        img, lst = a
        for code, _ in lst:
            img = by_code[code](img)
        return img
    res["host_callables_ms"] = median_ms(lambda: list(pool.map(callables, zip(prepared, ops))), max(5, args.reps // 2))
    res["mean_taps"] = [float(np.mean([plan.pool[int(x["h_bounds"]) + 1:int(x["h_bounds"]) + 2 * T:2].mean() for x in d])),
                        float(np.mean([plan.pool[int(x["v_bounds"]) + 1:int(x["v_bounds"]) + 2 * T:2].mean() for x in d]))]
    res["h_grid_fill"] = float(rows.mean() / rows.max())      # share of the horizontal pass's blocks that have work
    print(json.dumps(res), flush=True)

    # (d) fit_generator
    if not args.no_fit:
        from jpeg_detection_resnet_ssd_amd.keras import backend as K
        from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
        from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.networks.resnet_dct import ResNet50Custom
        K.clear_session()
        model = ResNet50Custom(weights=None, archi="deconv")
        model.compile(optimizer=SGD(lr=0.01, momentum=0.9, decay=1e-4, nesterov=True), loss="categorical_crossentropy")
        labels = [np.eye(1000, dtype=np.float32)[rng.integers(0, 1000, B)] for _ in batches]

        def gen(device_side):
            for i in itertools.cycle(range(len(batches))):
                if device_side:
                    yield prep(*batches[i]), labels[i]
                else:
                    yield jpeg_dct.emit_dct_inputs(host_pixels(batches[i]), deconv=True, n_threads=16), labels[i]
        order = [True, False, True, False] if have_pil else [True, True]
        rates = {True: [], False: []}
        for device_side in order:
            g = gen(device_side)
            model.fit_generator(g, steps_per_epoch=5, epochs=1, verbose=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.fit_generator(g, steps_per_epoch=args.fit_steps, epochs=1, verbose=0)
            torch.cuda.synchronize()
            rates[device_side].append(B * args.fit_steps / (time.perf_counter() - t0))
        res["fit_img_s_device_prep"] = rates[True]
        res["fit_img_s_host_prep"] = rates[False] if have_pil else "not measured (no PIL)"
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
