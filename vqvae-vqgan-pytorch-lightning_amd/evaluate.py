"""Evaluation entry point: the reference's ``vqvae/evaluate.py`` over ``MiniTrainer.test`` on one GPU.

    python vqvae-vqgan-pytorch-lightning_amd/evaluate.py --params_file example_confs/standard_vqvae.yaml \\
        --dataset_path test_images.pt --batch_size 32 --seed 0 --loading_path run/epoch=09.ckpt \\
        --fid_weights pt_inception-2015-12-05-6726825d.pth

The checkpoint is loaded as in reference evaluate.py:49 (``load_from_checkpoint(..., l_conf=None, t_conf=None,
init_cb=False, load_loss=False)``) and the test loop of vqvae/model.py:491-553 runs over the dataset: MSE, PSNR, SSIM, codebook
usage and perplexity, plus rFID when ``--fid_weights`` names the Inception weights (fid.py).  One JSON line of metrics is
printed.  ``--save_reconstructions DIR`` also writes every reconstruction as a PNG (the tensors the metrics read, through one HIP
kernel and host encode threads: imagelog.py); the metrics are the same with and without it.  The dataset is a DIRECTORY with the reference's layout -- its ``test/`` sub-folder is read in sorted file order
through ``data.get_datamodule`` with ``--workers`` decode threads -- or the tensor-file format train.py reads (``.pt`` / ``.npy``
of images [M,3,S,S] in [0,1]); the last batch may be short.  The ffcv loader is out of scope, as in train.py.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--params_file', type=str, required=True, help='yaml file with model params (example_confs/*.yaml)')
    p.add_argument('--dataloader', type=str, choices=['standard'], default='standard', help="'standard' = image folders (data.py)")
    p.add_argument('--dataset_path', type=str, required=True, help='directory holding a test/ image folder, or a .pt / .npy tensor of test images [M,3,S,S] in [0,1]')
    p.add_argument('--batch_size', type=int, required=True, help='evaluation is on one GPU')
    p.add_argument('--seed', type=int, required=True)
    p.add_argument('--loading_path', type=str, required=True, help='checkpoint to evaluate')
    p.add_argument('--workers', type=int, default=1, help='decode threads of the folder loader (at most 16 are used)')
    p.add_argument('--resize', choices=['squash', 'center_crop'], default='squash', help='folder loader geometry (train.py --resize)')
    p.add_argument('--fid_weights', type=str, default=None,
                   help='Inception weights for rFID (pt_inception-2015-12-05-6726825d.pth); omitted: no rfid')
    p.add_argument('--save_reconstructions', type=str, default=None, metavar='DIR',
                   help='write every reconstruction as DIR/<source file stem>.png (folder datasets) or DIR/<index:06d>.png '
                        '(tensor files); omitted: no images')
    p.add_argument('--save_grid_every', type=int, default=None, metavar='N',
                   help='with --save_reconstructions: also DIR/grids/batch=BBBBBB.png, ground truths over reconstructions, for '
                        'every N-th batch')
    p.add_argument('--dtype', choices=['bf16', 'f32', 'bf16x3'], default='bf16',
                   help='compute mode of the autoencoder (train.py --dtype); the FID network is always fp32')
    return p.parse_args(argv)


def load_images(path: str) -> torch.Tensor:
    data = torch.load(path) if path.endswith('.pt') else torch.from_numpy(__import__('numpy').load(path))
    data = data.float()
    if data.dim() != 4 or data.shape[1] != 3:
        raise SystemExit(f'evaluate.py: {path} holds {tuple(data.shape)}, expected images [M,3,S,S]')
    return data


def main(argv=None) -> dict:
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    args = parse_args(argv)
    train_mod = importlib.import_module(PKG + '.train')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    model_mod = importlib.import_module(PKG + '.model')
    if not torch.cuda.is_available():
        raise SystemExit('evaluate.py needs an MI355X: the test loop is HIP kernels only (no CPU fallback)')
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    torch.manual_seed(args.seed)
    conf = train_mod.get_model_conf(args.params_file)
    dtype = torch.bfloat16 if args.dtype == 'bf16' else 'bf16x3' if args.dtype == 'bf16x3' else torch.float32
    model = model_mod.VQVAE.load_from_checkpoint(args.loading_path, strict=False, image_size=int(conf['image_size']),
                                                 ae_conf=conf['autoencoder'], q_conf=conf['quantizer'], l_conf=None,
                                                 t_conf=None, init_cb=False, load_loss=False, compute_dtype=dtype)
    model = model.to(device)
    model.fid_weights = args.fid_weights
    b = args.batch_size
    if os.path.isdir(args.dataset_path):
        batches = importlib.import_module(PKG + '.data').get_datamodule(
            args.dataset_path, int(conf['image_size']), b, args.workers, args.seed, mode='test', device=device,
            resize=args.resize).test
    else:
        data = load_images(args.dataset_path)
        batches = [data[i:i + b].to(device) for i in range(0, data.shape[0], b)]
    if not len(batches):
        raise SystemExit(f'evaluate.py: {args.dataset_path} holds no images')
    saver = None
    if args.save_reconstructions is not None:
        imagelog = importlib.import_module(PKG + '.imagelog')
        if isinstance(batches, list):
            names = [f'{i:06d}.png' for i in range(data.shape[0])]
            per_batch = [names[i:i + b] for i in range(0, len(names), b)]
        else:
            stems = imagelog.unique_stems([batches.folder.path(i) for i in range(len(batches.folder))])
            per_batch = [[stems[i] + '.png' for i in ids] for ids in batches.epoch_batches()]
        saver = imagelog.ReconstructionSaver(imagelog.ImageWriter(args.save_reconstructions, workers=max(args.workers, 2)),
                                             per_batch, args.save_grid_every)
        model.reconstruction_sink = saver
    try:
        out = trainer_mod.MiniTrainer().test(model, batches)
    finally:
        model.reconstruction_sink = None
        if saver is not None:
            saver.close()
    if hasattr(batches, 'close'):
        batches.close()
    out = {k: float(v) for k, v in out.items()}
    print(json.dumps(out), flush=True)
    return out


if __name__ == '__main__':
    main()
