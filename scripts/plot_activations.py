#!/usr/bin/env python
"""Attention-map ("saliency") frames of a trained PoseNet on the MI355X path.

Command line of the reference's scripts/plot_activations.py (its lines 25-36: --dataset --scene --weights --config_file
--device --val --output_dir) and its flow: PoseNet in eval mode, batch size 1, per frame the gradient of pose.mean() with
respect to the image, saliency = max over channels of |gradient * image| scaled to [0, 1], jet colour map blended over the
un-normalised frame (lines 112-145).  The gradient and the map are computed on the device (PoseNet.saliency); the colour map
and the blend are host work (geomapnet_amd.evaluate.attention_overlay).  Additions: `--dataset Synthetic`
(+ `--synthetic_length --height --width --u8_input`), `--dtype` (default fp32: batch 1 is latency-bound, and the fp32 gradient
is the reference's).  Output: numbered PNG frames `<dataset>_<scene>_<model>_attention_%05d.png` (PIL), plus the reference's
`.avi` (XVID, 20 fps) when OpenCV is importable.
"""
import argparse
import configparser
import os
import os.path as osp
import sys

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser(description="Activation visualization script")
    parser.add_argument("--dataset", type=str, choices=("7Scenes", "RobotCar", "Synthetic"), default="Synthetic", help="Dataset")
    parser.add_argument("--scene", type=str, default="synthetic", help="Scene name")
    parser.add_argument("--weights", type=str, help="trained weights to load")
    parser.add_argument("--config_file", type=str, help="configuration file used for training")
    parser.add_argument("--device", type=str, default="0", help="GPU device(s)")
    parser.add_argument("--val", action="store_true", help="Use val split")
    parser.add_argument("--output_dir", type=str, required=True, help="Output directory for the frames (and the video)")
    # additions
    parser.add_argument("--dtype", choices=("fp32", "fp32x3", "fp16"), default="fp32",
                        help="compute precision of the forward and backward pass (default fp32)")
    parser.add_argument("--synthetic_length", type=int, default=16)
    parser.add_argument("--u8_input", action="store_true", help="frames as uint8 [H,W,3]; ToTensor + Normalize run on the "
                        "device (model.set_input_u8)")
    parser.add_argument("--device_resize", type=int, default=None, metavar="SIZE",
                        help="torchvision's Resize(SIZE) on the device (PIL's bilinear resample, bit for bit; the reference's "
                             "transform): the dataset yields frames of --height x --width and the network runs at the resized "
                             "size; needs --u8_input")
    parser.add_argument("--stats_file", type=str, default=None, metavar="PATH",
                        help="the Normalize constants of --u8_input from PATH, a stats.txt as scripts/dataset_mean.py writes it "
                             "(row 0 the mean, row 1 the variance) instead of the synthetic set's; needs --u8_input")
    parser.add_argument("--height", type=int, default=256)
    parser.add_argument("--width", type=int, default=341)
    return parser


def run(args, dataset=None, stats=None, _binding=None, log=print):
    """returns the list of PNG files written.  dataset: frames as (image, pose) pairs; stats: (mean[3], std[3]) of its Normalize
    (the scene's stats.txt in the reference; given, it takes the place of --stats_file)"""
    import numpy as np
    import torch
    from PIL import Image
    from torch.utils.data import DataLoader
    import geomapnet_amd as G
    from geomapnet_amd import evaluate as E
    from geomapnet_amd.data import SyntheticFrames

    if args.device_resize is not None and not args.u8_input:
        raise SystemExit("--device_resize needs --u8_input: Resize runs on the device's uint8 frames, before Normalize (fp32 frames "
                         "arrive normalised)")
    if args.stats_file is not None and not args.u8_input:
        raise SystemExit("--stats_file needs --u8_input: the statistics are those of uint8 frames, for the Normalize of the device's "
                         "input conversion (fp32 frames arrive normalised)")
    if "CUDA_VISIBLE_DEVICES" not in os.environ:
        os.environ["CUDA_VISIBLE_DEVICES"] = args.device
    G.set_compute_dtype(args.dtype)
    kw = {} if _binding is None else {"_binding": _binding}

    settings = configparser.ConfigParser()
    with open(args.config_file, "r") as f:
        settings.read_file(f)
    seed = settings.getint("training", "seed")
    dropout = settings["hyperparameters"].getfloat("dropout")

    # model
    feature_extractor = G.resnet34(pretrained=False, **kw)
    model = G.PoseNet(feature_extractor, droprate=dropout, pretrained=False, **kw)
    model.eval()
    if stats is not None:
        mean, std = stats
    elif args.stats_file is not None:
        mean, std = G.read_stats(args.stats_file)
    else:
        mean, std = SyntheticFrames.MEAN, SyntheticFrames.STD
    if args.u8_input:
        model.set_input_u8(mean, std)
    if args.device_resize is not None:
        model.set_input_resize(args.device_resize)

    # load weights
    weights_filename = osp.expanduser(args.weights)
    if not osp.isfile(weights_filename):
        log("Could not load weights from {:s}".format(weights_filename))
        sys.exit(-1)
    checkpoint = torch.load(weights_filename, map_location=lambda storage, loc: storage, weights_only=False)
    G.load_state_dict(model, checkpoint["model_state_dict"])
    log("Loaded weights from {:s}".format(weights_filename))

    # dataset
    train = not args.val
    log("Visualizing {:s} data".format("TRAIN" if train else "VAL"))
    if dataset is None:
        if args.dataset != "Synthetic":
            raise NotImplementedError(
                "the {:s} image reader is host-side file parsing outside the MI355X hot path: pass the frame dataset "
                "to run(args, dataset=...), or use --dataset Synthetic".format(args.dataset))
        dataset = SyntheticFrames(args.synthetic_length, H=args.height, W=args.width, seed=seed + (0 if train else 1),
                                  uint8=args.u8_input)

    # loader (batch_size MUST be 1)
    loader = DataLoader(dataset, batch_size=1, shuffle=False, num_workers=0, pin_memory=torch.cuda.is_available())
    CUDA = torch.cuda.is_available()
    torch.manual_seed(seed)
    if CUDA:
        model.cuda()

    out_dir = osp.expanduser(args.output_dir)
    os.makedirs(out_dir, exist_ok=True)
    model_name = "posenet" if args.weights.find("posenet") >= 0 else "vidvo"
    stem = "{:s}_{:s}_attention_{:s}".format(args.dataset, args.scene, model_name)
    vwrite = None
    try:
        import cv2
    except ImportError:
        cv2 = None

    files = []
    for batch_idx, (data, _) in enumerate(loader):
        if CUDA:
            data = data.cuda()
        _, maps = model.saliency(data)
        if args.device_resize is not None:  # the overlay is drawn on the frame the network saw: read it back from the plan's buffer
            eng = model._engine
            plan = eng.plan(0, 1, 1, *eng.image_dims(data), eng.source_dims(data))
            frame = eng.resized_frames(plan)[0].cpu().numpy()
        else:
            frame = data[0].cpu().numpy()
        img = E.attention_overlay(frame, maps[0].cpu().numpy(), mean, std)
        if cv2 is not None and vwrite is None:
            out_filename = osp.join(out_dir, stem + ".avi")
            vwrite = cv2.VideoWriter(out_filename, fourcc=cv2.VideoWriter_fourcc(*"XVID"), fps=20.0,
                                     frameSize=(img.shape[1], img.shape[0]))
            log("Initialized VideoWriter to {:s} with frames size {:d} x {:d}".format(out_filename, img.shape[1], img.shape[0]))
        if vwrite is not None:
            vwrite.write(img)
        fn = osp.join(out_dir, "{:s}_{:05d}.png".format(stem, batch_idx))
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(fn)  # PIL takes RGB
        files.append(fn)
        if batch_idx % 200 == 0:
            log("{:d} / {:d}".format(batch_idx, len(loader)))
    if vwrite is not None:
        vwrite.release()
        log("{:s} written".format(osp.join(out_dir, stem + ".avi")))
    log("{:d} frames written to {:s}".format(len(files), out_dir))
    return files


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.config_file is None or args.weights is None:
        build_parser().error("--config_file and --weights are required")
    run(args)


if __name__ == "__main__":
    main()
