"""Segment images of any size with a trained checkpoint: tiled, optionally test-time-augmented
prediction on the MI355X, then an optional clean-up of the mask (drop specks, fill holes).

    python predict.py --model models/unet_pde_regularized_ema.pth --input micrographs/ --output masks/
    python predict.py --model m.pth --input a.png --output out --tta d4 --min-object-area 20 --fill-holes

For every input image ``<stem>_mask.png`` (0 / 255, the input's own size) is written to --output, with
--save-prob also ``<stem>_prob.npy`` (float32 probabilities). With ``--refine {rd,pf} --refine-steps N``
the probabilities are evolved under the PDE before the threshold, and --save-prob saves the refined map.
"""
import argparse
import os
import sys
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".tif", ".tiff", ".bmp")


def _int_in(lo, hi, what):
    def parse(text):
        n = int(text)
        if not lo <= n <= hi:
            raise argparse.ArgumentTypeError(f"{text}: {what} in [{lo}, {hi}] is needed")
        return n
    return parse


def _tile(text):
    n = int(text)
    if not 16 <= n <= 2048 or n % 16:
        raise argparse.ArgumentTypeError(f"{text}: a multiple of 16 in [16, 2048] is needed")
    return n


def _threshold(text):
    v = float(text)
    if not 0.0 <= v < 1.0:
        raise argparse.ArgumentTypeError(f"{text}: a threshold in [0, 1) is needed")
    return v


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Segment images of any size with a trained U-Net checkpoint")
    ap.add_argument("--model", type=str, required=True, help="checkpoint (state_dict) of the U-Net")
    ap.add_argument("--input", type=str, required=True, help="an image file, or a directory of images")
    ap.add_argument("--output", type=str, required=True, help="directory for the masks")
    ap.add_argument("--tile", type=_tile, default=512,
                    help="largest tile side, a multiple of 16 in [16, 2048] (default: 512)")
    ap.add_argument("--overlap", type=_int_in(0, 256, "an overlap"), default=64,
                    help="overlap of neighbouring tiles in pixels, at most half the tile (default: 64)")
    ap.add_argument("--tta", choices=["none", "flip", "d4"], default="none",
                    help="test-time augmentation: average over the 4 flips or all 8 symmetries (default: none)")
    ap.add_argument("--threshold", type=_threshold, default=0.5, help="mask = probability > threshold (default: 0.5)")
    ap.add_argument("--min-object-area", type=_int_in(0, 1 << 30, "an area"), default=0, metavar="N",
                    help="drop predicted objects below N pixels (default: 0)")
    ap.add_argument("--fill-holes", action="store_true", help="fill the holes of the predicted objects")
    ap.add_argument("--connectivity", type=int, choices=[4, 8], default=8,
                    help="pixel connectivity of an object for the clean-up (default: 8)")
    ap.add_argument("--save-prob", action="store_true", help="also write <stem>_prob.npy")
    ap.add_argument("--resize", type=_int_in(1, 32768, "a side"), nargs=2, default=None, metavar=("H", "W"),
                    help="resize every image to H x W (bilinear) before predicting and the mask back (nearest): "
                         "for models trained at one fixed size")
    from physics_informed_image_segmentation_amd.pde import add_refine_flags, refine_from_args
    add_refine_flags(ap)
    args = ap.parse_args(argv)
    args.refine_preset = refine_from_args(ap, args)
    if args.overlap > args.tile // 2:
        ap.error(f"--overlap {args.overlap}: at most half the tile ({args.tile // 2}) is allowed")
    if not Path(args.model).is_file():
        ap.error(f"--model {args.model}: no such file")
    src = Path(args.input)
    if src.is_dir():
        args.files = sorted(p for p in src.iterdir() if p.suffix.lower() in IMAGE_SUFFIXES)
        if not args.files:
            ap.error(f"--input {args.input}: no image ({', '.join(IMAGE_SUFFIXES)}) in the directory")
    elif src.is_file():
        args.files = [src]
    else:
        ap.error(f"--input {args.input}: no such file or directory")
    return args


def main(argv=None):
    args = parse_args(argv)  # bad arguments end here, before the GPU is touched
    import numpy as np
    import torch
    from PIL import Image

    from physics_informed_image_segmentation_amd.evaluate_comparison import load_model
    from physics_informed_image_segmentation_amd.predict import Predictor, clean_mask
    if not torch.cuda.is_available():
        raise SystemExit("predict.py: needs the GPU (this build has no CPU fallback)")
    device = torch.device("cuda")
    model = load_model(Path(args.model), device)
    predictor = Predictor(model, tile=args.tile, overlap=args.overlap, tta=None if args.tta == "none" else args.tta,
                          threshold=args.threshold, refine=args.refine_preset)
    out_dir = Path(args.output)
    out_dir.mkdir(parents=True, exist_ok=True)
    written = []
    for path in args.files:
        img = Image.open(path).convert("L")
        size = img.size  # (W, H)
        if args.resize is not None:
            img = img.resize((args.resize[1], args.resize[0]), resample=Image.BILINEAR)
        prob, mask = predictor.predict_image(np.asarray(img, dtype=np.uint8))
        if args.min_object_area > 1 or args.fill_holes:
            mask = clean_mask(mask, min_area=args.min_object_area, fill_holes=args.fill_holes,
                              connectivity=args.connectivity)
        out = Image.fromarray((mask.cpu().numpy() * 255).astype(np.uint8))
        if out.size != size:
            out = out.resize(size, resample=Image.NEAREST)
        mask_path = out_dir / f"{path.stem}_mask.png"
        out.save(mask_path)
        if args.save_prob:
            np.save(out_dir / f"{path.stem}_prob.npy", prob.cpu().numpy())
        written.append(mask_path)
        print(f"{path.name}: {size[1]} x {size[0]} -> {mask_path}")
    return written


if __name__ == "__main__":
    main()
