"""Copy a tree of class directories with every image pre-sized for the coefficient generators
(vgg_jpeg_keras/generators/coefficient_generators.py): resized so that its shorter side is `--side`, centre-cropped to
side x side and saved as a baseline 4:2:0 JPEG -- the files those generators accept, whose own coefficients then reach the
models without being decoded to pixels again.  Host only; needs Pillow.

    python tools/presize_dataset.py SRC DST [--side 256] [--resample BICUBIC] [--quality 90] [--workers 8]
                                    [--restart-rows N | --restart-mcus N]

SRC/<class>/<image> becomes DST/<class>/<image stem>.jpg; files Pillow cannot open are reported and skipped.  `--side`
should be a multiple of 16 and at least the generators' `target_length`: only whole MCUs of a file are eligible for a window.
`--restart-rows N` writes a restart marker every N MCU rows, `--restart-mcus N` every N MCUs (one or the other): such files
can be entropy-decoded on the GPU (`device_entropy=True` / DJ_DEVICE_ENTROPY=1), one restart interval per lane, at the
price of two bytes and some padding bits per interval.  With neither, the files are what they always were."""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

RESAMPLE = ("NEAREST", "BOX", "BILINEAR", "HAMMING", "BICUBIC", "LANCZOS")


def presize(src, dst, side, resample, quality, restart_rows=0, restart_mcus=0):
    """One image: shorter side to `side` (the longer one rounded), centre crop, baseline 4:2:0 JPEG at `quality`, with a
    restart marker every `restart_rows` MCU rows or every `restart_mcus` MCUs when one of them is given."""
    from PIL import Image
    with Image.open(src) as im:
        im = im.convert("RGB")
        width, height = im.size
        ratio = side / min(width, height)
        width, height = max(side, int(round(width * ratio))), max(side, int(round(height * ratio)))
        im = im.resize((width, height), getattr(Image, resample))
        left, top = (width - side) // 2, (height - side) // 2
        im = im.crop((left, top, left + side, top + side))
        restart = {}
        if restart_rows:
            restart["restart_marker_rows"] = int(restart_rows)
        elif restart_mcus:
            restart["restart_marker_blocks"] = int(restart_mcus)
        im.save(dst, "JPEG", quality=quality, subsampling=2, progressive=False, optimize=False, **restart)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--resample", default="BICUBIC", choices=RESAMPLE)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--workers", type=int, default=8)
    restart = ap.add_mutually_exclusive_group()
    restart.add_argument("--restart-rows", type=int, default=0, metavar="N", help="a restart marker every N MCU rows")
    restart.add_argument("--restart-mcus", type=int, default=0, metavar="N", help="a restart marker every N MCUs")
    args = ap.parse_args(argv)
    if args.restart_rows < 0 or args.restart_mcus < 0:
        ap.error("--restart-rows / --restart-mcus must be positive")
    if args.side < 16 or args.side % 16:
        print("warning: --side %d is no multiple of 16: the last partial MCU of every file is never part of a window" % args.side,
              file=sys.stderr)
    jobs = []
    for name in sorted(os.listdir(args.src)):
        directory = os.path.join(args.src, name)
        if os.path.isdir(directory):
            os.makedirs(os.path.join(args.dst, name), exist_ok=True)
            for image in sorted(os.listdir(directory)):
                jobs.append((os.path.join(directory, image),
                             os.path.join(args.dst, name, os.path.splitext(image)[0] + ".jpg")))

    def work(job):
        try:
            presize(job[0], job[1], args.side, args.resample, args.quality, args.restart_rows, args.restart_mcus)
            return None
        except Exception as e:          # an unreadable file must not stop the copy of a dataset
            return "%s: %s" % (job[0], e)
    with ThreadPoolExecutor(max(1, args.workers)) as pool:
        failed = [r for r in pool.map(work, jobs) if r is not None]
    for line in failed:
        print("skipped " + line, file=sys.stderr)
    print("%d files written to %s, %d skipped" % (len(jobs) - len(failed), args.dst, len(failed)))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
