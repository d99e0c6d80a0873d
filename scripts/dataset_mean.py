#!/usr/bin/env python
"""Computes the mean and std of pixels in a dataset, on the device.

Command line of the reference's scripts/dataset_mean.py (--dataset --scene) and its output: `stats.txt`, row 0 the per-channel mean,
row 1 the per-channel VARIANCE of the pixels in ToTensor's [0, 1] units (`np.savetxt(..., fmt='%8.7f')`), the file the reference's
train.py / eval.py / plot_activations.py read their Normalize from (std = sqrt(row 1)) and `--stats_file` of this project's scripts
reads.  Where the reference walks the training split through a DataLoader and accumulates per-pixel float sums in numpy, the frames
are summed here as integers by one bandwidth-bound kernel (geomapnet_amd.pixel_sums, csrc/frame_stats.h), after the device's own Resize
when `--device_resize` is given -- the frames the network sees.  Differences, all additive:

* `--dataset Synthetic` (the only image source that ships; `--synthetic_length --height --width --seed` size it): for 7Scenes /
  RobotCar build the uint8 frame dataset yourself and call `run(args, dataset=...)`.
* `--device_resize SIZE`: torchvision's Resize(SIZE) first (the reference's transform has Resize(256)).
* `--output PATH` (default ./stats.txt; the reference writes ../data/<dataset>/<scene>/stats.txt).
* whole frames are counted: the reference's RandomCrop(crop_size) is not applied.
* "Std. pixel" prints the standard deviation (the reference prints the variance under that label); the FILE holds the variance.
"""
import argparse
import os
import os.path as osp
import sys

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser(description="Dataset images statistics")
    parser.add_argument("--dataset", type=str, choices=("7Scenes", "RobotCar", "Synthetic"), default="Synthetic", help="Dataset")
    parser.add_argument("--scene", type=str, default="synthetic", help="Scene name")
    # additions
    parser.add_argument("--device", type=str, default="0", help="value to be set to $CUDA_VISIBLE_DEVICES")
    parser.add_argument("--synthetic_length", type=int, default=1024, help="frames in the synthetic sequence")
    parser.add_argument("--height", type=int, default=256)
    parser.add_argument("--width", type=int, default=341)
    parser.add_argument("--seed", type=int, default=7, help="seed of the synthetic sequence ([training] seed of the other scripts)")
    parser.add_argument("--device_resize", type=int, default=None, metavar="SIZE",
                        help="torchvision's Resize(SIZE) on the device before the statistics are taken (PIL's bilinear resample, bit "
                             "for bit): the dataset yields frames of --height x --width")
    parser.add_argument("--batch_frames", type=int, default=192, help="frames per chunk staged to the device")
    parser.add_argument("--output", type=str, default="stats.txt", help="file to write (default ./stats.txt)")
    return parser


def run(args, dataset=None, _binding=None, log=print):
    """writes the file and returns its path.  dataset: (uint8 [h,w,3] frame, pose) items, a ResidentFrames view or a device tensor
    of frames; `_binding` (tests) substitutes another build of the kernel library for libmapnet_hip.so."""
    if "CUDA_VISIBLE_DEVICES" not in os.environ:
        os.environ["CUDA_VISIBLE_DEVICES"] = args.device
    import geomapnet_amd as G
    from geomapnet_amd.data import SyntheticFrames

    kw = {} if _binding is None else {"_binding": _binding}
    if dataset is None:
        if args.dataset != "Synthetic":
            raise NotImplementedError(
                "the {:s} image reader is host-side file parsing outside the MI355X hot path: pass the frame dataset "
                "to run(args, dataset=...), or use --dataset Synthetic".format(args.dataset))
        dataset = SyntheticFrames(args.synthetic_length, H=args.height, W=args.width, seed=args.seed, uint8=True)
    sums = G.pixel_sums(dataset, resize=args.device_resize, batch_frames=args.batch_frames, **kw)
    log("Mean pixel = {}".format(sums.mean()))
    log("Std. pixel = {}".format(sums.std()))
    parent = osp.dirname(osp.abspath(args.output))
    os.makedirs(parent, exist_ok=True)
    G.write_stats(args.output, sums)
    log("{:s} written".format(args.output))
    return args.output


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
