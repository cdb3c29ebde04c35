"""CLI of the reference (main.py:5-102): same flags and defaults, training on
the MI355X path. Build-only flags: --synthetic N_TRAIN N_VAL H W, --base-dir,
--device-cache, --augment {flip,d4,affine}, --clip-grad-norm FLOAT,
--skip-nonfinite, --ema-decay FLOAT, --no-ema-warmup, --pde-layer {rd,pf} with
--pde-layer-steps N and --pde-layer-{dt,mu,diffusion,threshold-a,epsilon},
--pde-layer-learn NAME [NAME ...] with --pde-layer-lr F."""
import argparse

from physics_informed_image_segmentation_amd.pde import (add_learn_flags, add_refine_flags, learn_from_args,
                                                         refine_from_args)
from physics_informed_image_segmentation_amd.train import train


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Train PDE-constrained cell segmentation model")
    p.add_argument("--single-stage", action="store_true",
                   help="Use single-stage training (PDE from start) instead of two-stage")
    p.add_argument("--pde-weight", type=float, default=1e-4, help="Weight for PDE regularization λ_RD")
    p.add_argument("--diffusion-coeff", type=float, default=5.0, help="Diffusion coefficient D for PDE")
    p.add_argument("--reaction-threshold", type=float, default=0.5, help="Reaction term threshold a for PDE")
    p.add_argument("--phase-field-weight", type=float, default=1e-4, help="Weight for phase-field energy λ_PF")
    p.add_argument("--epsilon", type=float, default=0.05, help="Interface width parameter ε")
    p.add_argument("--batch-size", type=int, default=8, help="Batch size per GPU")
    p.add_argument("--learning-rate", type=float, default=1e-4, help="Learning rate for AdamW")
    p.add_argument("--stage1-epochs", type=int, default=50, help="Maximum epochs for Stage I")
    p.add_argument("--stage2-epochs", type=int, default=50, help="Maximum epochs for Stage II")
    p.add_argument("--early-stopping-patience", type=int, default=5, help="Patience for early stopping")
    p.add_argument("--train-fraction", type=float, default=None, help="Fraction of training data to use")
    p.add_argument("--seed", type=int, default=42, help="Random seed")
    p.add_argument("--synthetic", type=int, nargs=4, metavar=("N_TRAIN", "N_VAL", "H", "W"), default=None,
                   help="train on the synthetic disc generator instead of images/")
    p.add_argument("--base-dir", type=str, default=None, help="directory holding images/, output/, models/")
    p.add_argument("--device-cache", action="store_true",
                   help="preprocess the datasets once and serve every batch from a device-resident cache "
                        "(with --synthetic: the host disc dataset, cached, instead of the on-GPU generator)")
    p.add_argument("--augment", choices=["flip", "d4", "affine"], default=None,
                   help="random flips / all 8 grid symmetries / a random rotation, scale, shift, flip and "
                        "brightness per sample and epoch on the training loader (needs --device-cache)")
    p.add_argument("--clip-grad-norm", type=float, default=None, metavar="FLOAT",
                   help="clip the global L2 norm of the gradients to FLOAT inside the fused AdamW step (default: off)")
    p.add_argument("--skip-nonfinite", action="store_true",
                   help="skip an optimizer step whose gradient norm is Inf or NaN (default: off)")
    p.add_argument("--ema-decay", type=float, default=None, metavar="FLOAT",
                   help="keep an exponential moving average of the weights with decay FLOAT in (0, 1) inside the "
                        "fused AdamW step; validation, early stopping and evaluation use it (default: off)")
    p.add_argument("--no-ema-warmup", action="store_true",
                   help="use --ema-decay from the first step instead of min(decay, (1 + k) / (10 + k))")
    add_refine_flags(p, prefix="pde-layer")
    add_learn_flags(p)
    a = p.parse_args(argv)
    a.pde_layer_refine = refine_from_args(p, a, prefix="pde-layer")
    a.pde_layer_learn, a.pde_layer_lr = learn_from_args(p, a, a.pde_layer_refine)
    if a.clip_grad_norm is not None and not a.clip_grad_norm > 0:
        p.error("--clip-grad-norm must be positive")
    if a.ema_decay is not None and not 0.0 < a.ema_decay < 1.0:
        p.error("--ema-decay must be in (0, 1)")
    if a.augment and not a.device_cache:
        p.error("--augment needs --device-cache")
    return a


def main(argv=None):
    a = parse_args(argv)
    return train(use_two_stage=not a.single_stage, pde_weight=a.pde_weight, diffusion_coeff=a.diffusion_coeff,
                 reaction_threshold=a.reaction_threshold, phase_field_weight=a.phase_field_weight,
                 epsilon=a.epsilon, batch_size=a.batch_size, learning_rate=a.learning_rate,
                 stage1_epochs=a.stage1_epochs, stage2_epochs=a.stage2_epochs,
                 early_stopping_patience=a.early_stopping_patience, train_fraction=a.train_fraction,
                 seed=a.seed, base_dir=a.base_dir,
                 synthetic=tuple(a.synthetic) if a.synthetic else None,
                 device_data=not a.device_cache, device_cache=a.device_cache, augment=a.augment,
                 max_grad_norm=a.clip_grad_norm, skip_nonfinite=a.skip_nonfinite,
                 ema_decay=a.ema_decay, ema_warmup=not a.no_ema_warmup,
                 pde_layer=a.pde_layer_refine,
                 **({} if a.pde_layer_learn is None else {"pde_layer_learn": a.pde_layer_learn,
                                                          "pde_layer_lr": a.pde_layer_lr}))


if __name__ == "__main__":
    main()
