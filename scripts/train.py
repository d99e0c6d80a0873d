#!/usr/bin/env python
"""Training script for PoseNet and the MapNet variants on the MI355X hot path.

Command line of the reference's scripts/train.py (/root/reference/scripts/train.py:25-43: --dataset --scene
--config_file --model --device --checkpoint --learn_beta --learn_gamma --resume_optim --suffix) and the same
construction order: model, criterion, optimizer with the criterion scalars as extra parameter groups, datasets,
Trainer.train_val.  Differences, all additive:

* `--dataset Synthetic` (the only image source that ships: the 7Scenes / RobotCar readers are host-side file
  parsers outside the hot path -- pass your own Dataset objects to `run(..., datasets=(train, val))`);
  `--synthetic_length`, `--height`, `--width` size it.
* `--dtype fp16|fp32` selects the compute precision of the HIP kernels (fp16 storage + fp32 accumulate, or the
  fp32 parity build).
* `--epochs`, `--batch_size`, `--logdir` override the config file (smoke runs).
* `--stats_file PATH` / `--stats_from_frames` (with `--u8_input`): the Normalize constants from a stats.txt (the reference's
  train.py:126-127), or computed from the training frames on the device before training and written to <logdir>/stats.txt.
* launched under `python -m torch.distributed.run --nproc-per-node N scripts/train.py ...` it trains data
  parallel: one process per GPU, windows sharded, gradient buckets all-reduced over RCCL during backward.
"""
import argparse
import configparser
import json
import os
import os.path as osp
import sys

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    # one rank of a data-parallel job (torch.distributed.run): the RCCL channel budget, before torch loads the HIP runtime
    os.environ.setdefault("NCCL_MIN_NCHANNELS", "4")
    os.environ.setdefault("NCCL_MAX_NCHANNELS", "8")


def build_parser():
    parser = argparse.ArgumentParser(description="Training script for PoseNet and MapNet variants")
    parser.add_argument("--dataset", type=str, choices=("7Scenes", "RobotCar", "Synthetic"), default="Synthetic",
                        help="Dataset")
    parser.add_argument("--scene", type=str, default="synthetic", help="Scene name")
    parser.add_argument("--config_file", type=str, help="configuration file")
    parser.add_argument("--model", choices=("posenet", "mapnet", "mapnet++"), help="Model to train")
    parser.add_argument("--device", type=str, default="0", help="value to be set to $CUDA_VISIBLE_DEVICES")
    parser.add_argument("--checkpoint", type=str, help="Checkpoint to resume from", default=None)
    parser.add_argument("--learn_beta", action="store_true", help="Learn the weight of translation loss")
    parser.add_argument("--learn_gamma", action="store_true", help="Learn the weight of rotation loss")
    parser.add_argument("--resume_optim", action="store_true",
                        help="Resume optimization (only effective if a checkpoint is given")
    parser.add_argument("--suffix", type=str, default="", help="Experiment name suffix (as is)")
    # additions
    parser.add_argument("--dropout_active", action="store_true",
                        help="apply the config's dropout on the device in training mode (default: identity, the reference's "
                             "behaviour under its pinned PyTorch 0.4.1)")
    parser.add_argument("--dtype", choices=("fp16", "fp16x2m", "fp16x2q", "fp16x2", "fp32x3", "fp32"), default="fp16x2m",
                        help="compute precision of the HIP kernels.  Default fp16x2m: the reference computes in fp32 "
                             "(common/train.py:322-363) and this is the fastest mode whose loss and poses match it to 1e-4 / 1e-3 "
                             "(split-fp16 forward pass, single-fp16 backward pass).  fp16 is 1.5x faster and trains to the same "
                             "accuracy on the synthetic scene (profiles/r05) but deviates 1.3e-2 on the poses of a single step; fp16x2 "
                             "/ fp32x3 / fp32 keep fp32-class arithmetic in the backward pass too; fp16x2q is EXPERIMENTAL (forward cross terms from fp8 "
                             "copies with fixed exponents: they saturate silently beyond |activation| 448 / |weight| 7, poses 6e-4 from the "
                             "reference, gradients off by percents -- not for pretrained or diverging networks)")
    parser.add_argument("--pretrained", choices=("auto", "yes", "no"), default="auto",
                        help="start from the torchvision ImageNet ResNet-34 ($TORCH_MODEL_ZOO/resnet34-333f7ec4.pth, as the "
                             "reference does: models.resnet34(pretrained=True), scripts/train.py:76) and re-initialise only the "
                             "three linear layers; auto = yes when that file exists (there is no network to fetch it)")
    parser.add_argument("--synthetic_length", type=int, default=1024, help="frames in the synthetic sequence")
    parser.add_argument("--synthetic_val_length", type=int, default=None, help="frames in the validation sequence "
                        "(default: a quarter of --synthetic_length)")
    parser.add_argument("--u8_input", action="store_true", help="frames as uint8 [H,W,3]; ToTensor + Normalize run on the "
                        "device (model.set_input_u8)")
    parser.add_argument("--device_color_jitter", action="store_true",
                        help="apply the config's color_jitter as torchvision's ColorJitter(cj, cj, cj, hue=0.5) on the device, "
                             "to training and validation frames (the reference's transform, scripts/train.py:121-125); needs "
                             "--u8_input.  Without this flag color_jitter is read and not applied")
    parser.add_argument("--device_resize", type=int, default=None, metavar="SIZE",
                        help="torchvision's Resize(SIZE) on the device (PIL's bilinear resample, bit for bit; the reference's "
                             "transform, scripts/train.py:120): the dataset yields frames of --height x --width and the network runs "
                             "at the resized size; needs --u8_input")
    parser.add_argument("--stats_file", type=str, default=None, metavar="PATH",
                        help="the Normalize constants of --u8_input from PATH, a stats.txt as scripts/dataset_mean.py writes it "
                             "(row 0 the mean, row 1 the variance; the reference's train.py:126-127) instead of the synthetic set's; "
                             "needs --u8_input")
    parser.add_argument("--stats_from_frames", action="store_true",
                        help="compute the Normalize constants from the training frames before training, on the device "
                             "(geomapnet_amd.pixel_sums; through --device_resize first when that is given), log them, write "
                             "stats.txt into the log directory and use them; needs --u8_input, excludes --stats_file")
    parser.add_argument("--resident_frames", action="store_true",
                        help="upload the training and validation frames once into one device tensor and gather every batch from "
                             "it by index on the device (geomapnet_amd/resident.py) instead of stacking frames on the host every "
                             "step; the batch order is the host loader's.  Works with or without --u8_input, --device_resize, "
                             "--device_color_jitter; the store must fit the device's free memory")
    parser.add_argument("--fused_eval", action="store_true",
                        help="run the validation passes as the fused inference pass (model.set_eval_fused: BatchNorm, residual and "
                             "ReLU in the epilogues of the convolutions; the same poses bit for bit); training passes are "
                             "untouched.  --dtype fp16x2m or fp16x2")
    kinds = ("l1", "mse", "smooth_l1", "huber", "quaternion")
    parser.add_argument("--t_loss_fn", choices=kinds, default="l1",
                        help="the training criterion's t_loss_fn (common/criterion.py:34,55,112; the reference's scripts pass "
                             "none, i.e. nn.L1Loss): l1, mse, smooth_l1 (beta = --loss_param), huber (delta = --loss_param), all "
                             "evaluated in the fused criterion kernel; quaternion is a rotation loss and is refused here")
    parser.add_argument("--q_loss_fn", choices=kinds, default="l1",
                        help="the training criterion's q_loss_fn: as --t_loss_fn, or quaternion (QuaternionLoss, "
                             "common/criterion.py:15-31).  The validation criterion keeps L1 for both, as in the reference")
    parser.add_argument("--loss_param", type=float, default=1.0, help="beta of smooth_l1 / delta of huber")
    parser.add_argument("--height", type=int, default=256)
    parser.add_argument("--width", type=int, default=341)
    parser.add_argument("--epochs", type=int, default=None, help="override [training] n_epochs")
    parser.add_argument("--batch_size", type=int, default=None, help="override [training] batch_size")
    parser.add_argument("--num_workers", type=int, default=None, help="override [training] num_workers")
    parser.add_argument("--logdir", type=str, default=None, help="checkpoint directory (default logs/<experiment>)")
    return parser


def _init_distributed():
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        local = int(os.environ.get("LOCAL_RANK", "0"))
        if torch.cuda.is_available():
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")
    return world


def _rank():
    """data-parallel rank (0 outside a launcher): mixed into the dropout key so that replicas do not draw identical masks"""
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else int(os.environ.get("RANK", "0"))


def run(args, datasets=None, _binding=None, log=print):
    """builds everything the reference's script builds and runs Trainer.train_val; returns the Trainer.
    `_binding` (tests) substitutes another build of the kernel library for libmapnet_hip.so."""
    import torch
    import geomapnet_amd as G
    from geomapnet_amd.data import MF, MFOnline, SyntheticFrames
    from geomapnet_amd.trainer import Trainer

    _init_distributed()
    G.set_compute_dtype(args.dtype)
    kw = {} if _binding is None else {"_binding": _binding}

    settings = configparser.ConfigParser()
    with open(args.config_file, "r") as f:
        settings.read_file(f)
    if args.epochs is not None:
        settings["training"]["n_epochs"] = str(args.epochs)
    if args.batch_size is not None:
        settings["training"]["batch_size"] = str(args.batch_size)
    if args.num_workers is not None:
        settings["training"]["num_workers"] = str(args.num_workers)
    section = settings["optimization"]
    optim_config = {k: json.loads(v) for k, v in section.items() if k != "opt"}
    opt_method = section["opt"]
    lr = optim_config.pop("lr")
    weight_decay = optim_config.pop("weight_decay")

    section = settings["hyperparameters"]
    dropout = section.getfloat("dropout")
    color_jitter = section.getfloat("color_jitter", 0)
    sax = 0.0
    saq = section.getfloat("beta")
    mapnet = args.model.find("mapnet") >= 0
    online = args.model.find("++") >= 0
    if mapnet:
        skip = section.getint("skip")
        real = section.getboolean("real")
        variable_skip = section.getboolean("variable_skip")
        srx = 0.0
        srq = section.getfloat("gamma")
        steps = section.getint("steps")
    if online:
        vo_lib = section.get("vo_lib", "orbslam")
        log("Using {:s} VO".format(vo_lib))
    seed = settings["training"].getint("seed")

    # model (random initialisation: there is no model zoo offline; load weights with --checkpoint)
    torch.manual_seed(seed)
    zoo_file = os.path.join(os.environ.get("TORCH_MODEL_ZOO", os.path.join("..", "data", "models")), "resnet34-333f7ec4.pth")
    pretrained = args.pretrained == "yes" or (args.pretrained == "auto" and os.path.isfile(zoo_file))
    print("ResNet-34 weights: %s" % ("ImageNet (%s)" % zoo_file if pretrained else "random initialisation"))
    feature_extractor = G.resnet34(pretrained=pretrained, **kw)
    posenet = G.PoseNet(feature_extractor, droprate=dropout, pretrained=pretrained, filter_nans=(args.model == "mapnet++"),
                        dropout_active=args.dropout_active, dropout_seed=seed ^ (_rank() << 32), **kw)
    model = posenet if args.model == "posenet" else G.MapNet(mapnet=posenet)

    if args.stats_file is not None and args.stats_from_frames:
        raise SystemExit("--stats_file and --stats_from_frames exclude each other: one reads the Normalize constants, the other "
                         "computes them")
    if (args.stats_file is not None or args.stats_from_frames) and not args.u8_input:
        raise SystemExit("%s needs --u8_input: the statistics are those of uint8 frames, for the Normalize of the device's input "
                         "conversion (fp32 frames arrive normalised)" % ("--stats_file" if args.stats_file is not None
                                                                        else "--stats_from_frames"))
    if args.u8_input:  # the DataLoader ships decoded frames; normalisation happens in the input-conversion kernel
        if args.stats_file is not None:
            model.set_input_u8(*G.read_stats(args.stats_file))
        else:  # (--stats_from_frames replaces these once the training frames exist, below)
            model.set_input_u8(SyntheticFrames.MEAN, SyntheticFrames.STD)
    if args.device_resize is not None:
        if not args.u8_input:
            raise SystemExit("--device_resize needs --u8_input: Resize runs on the device's uint8 frames, before Normalize (fp32 "
                             "frames arrive normalised)")
        model.set_input_resize(args.device_resize)
    if args.fused_eval:  # (governs eval-mode forward passes only: the validation half of Trainer.train_val)
        model.set_eval_fused(True)
    if args.device_color_jitter and color_jitter > 0:
        assert color_jitter <= 1.0
        if not args.u8_input:
            raise SystemExit("--device_color_jitter needs --u8_input: ColorJitter runs in the device's uint8 input conversion, "
                             "before Normalize (fp32 frames arrive normalised)")
        log("Using ColorJitter data augmentation")
        model.set_color_jitter(color_jitter, color_jitter, color_jitter, 0.5, seed=seed ^ (_rank() << 32))

    # loss function
    def loss_module(name):
        return {"l1": torch.nn.L1Loss, "mse": torch.nn.MSELoss, "quaternion": G.QuaternionLoss,
                "smooth_l1": lambda: torch.nn.SmoothL1Loss(beta=args.loss_param),
                "huber": lambda: torch.nn.HuberLoss(delta=args.loss_param)}[name]()

    fkw = dict(t_loss_fn=loss_module(args.t_loss_fn), q_loss_fn=loss_module(args.q_loss_fn))
    if args.model == "posenet":
        train_criterion = G.PoseNetCriterion(sax=sax, saq=saq, learn_beta=args.learn_beta, **fkw, **kw)
        val_criterion = G.PoseNetCriterion(**kw)
    else:
        ckw = dict(sax=sax, saq=saq, srx=srx, srq=srq, learn_beta=args.learn_beta, learn_gamma=args.learn_gamma, **fkw, **kw)
        if online:
            train_criterion = G.MapNetOnlineCriterion(gps_mode=(vo_lib == "gps"), **ckw)
            val_criterion = G.MapNetOnlineCriterion(**kw)
        else:
            train_criterion = G.MapNetCriterion(**ckw)
            val_criterion = G.MapNetCriterion(**kw)

    # optimizer
    param_list = [{"params": model.parameters()}]
    if args.learn_beta and hasattr(train_criterion, "sax") and hasattr(train_criterion, "saq"):
        param_list.append({"params": [train_criterion.sax, train_criterion.saq]})
    if args.learn_gamma and hasattr(train_criterion, "srx") and hasattr(train_criterion, "srq"):
        param_list.append({"params": [train_criterion.srx, train_criterion.srq]})
    optimizer = G.Optimizer(params=param_list, method=opt_method, base_lr=lr, weight_decay=weight_decay, **optim_config)

    # datasets
    if datasets is not None:
        train_frames, val_frames = datasets
    elif args.dataset == "Synthetic":
        train_frames = SyntheticFrames(args.synthetic_length, H=args.height, W=args.width, seed=seed, uint8=args.u8_input)
        n_val = args.synthetic_val_length if args.synthetic_val_length else max(args.synthetic_length // 4, 8)
        val_frames = SyntheticFrames(n_val, H=args.height, W=args.width, seed=seed + 1, uint8=args.u8_input)
    else:
        raise NotImplementedError(
            "the {:s} image reader is host-side file parsing outside the MI355X hot path: build the frame datasets "
            "yourself and call run(args, datasets=(train, val)), or use --dataset Synthetic".format(args.dataset))
    if args.model == "posenet":
        train_set, val_set = train_frames, val_frames
    elif online:
        train_set = MFOnline(train_frames, val_frames, gps_mode=(vo_lib == "gps"), val_gt_dataset=val_frames, steps=steps,
                             skip=skip, variable_skip=variable_skip)
        val_set = None
    else:
        mkw = dict(steps=steps, skip=skip, variable_skip=variable_skip, real=real)
        train_set = MF(train_frames, train=True, **mkw)
        val_set = MF(val_frames, train=False, **mkw)

    # trainer
    config_name = args.config_file.split("/")[-1].split(".")[0]
    experiment_name = "{:s}_{:s}_{:s}_{:s}".format(args.dataset, args.scene, args.model, config_name)
    if args.learn_beta:
        experiment_name = "{:s}_learn_beta".format(experiment_name)
    if args.learn_gamma:
        experiment_name = "{:s}_learn_gamma".format(experiment_name)
    experiment_name += args.suffix
    if args.stats_from_frames:  # the statistics of the frames the network will see: after the device's Resize, whole frames
        sums = G.pixel_sums(train_frames, resize=args.device_resize, **kw)
        logdir = args.logdir if args.logdir is not None else osp.join(os.getcwd(), "logs", experiment_name)
        stats_path = osp.join(logdir, "stats.txt")
        if _rank() == 0:
            os.makedirs(logdir, exist_ok=True)
            G.write_stats(stats_path, sums)
            log("Mean pixel = {}".format(sums.mean()))
            log("Std. pixel = {}".format(sums.std()))
            log("{:s} written".format(stats_path))
        model.set_input_u8(sums.mean(), sums.std())
    trainer = Trainer(model, optimizer, train_criterion, settings, experiment_name, train_set, val_set, device=args.device,
                      checkpoint_file=args.checkpoint, resume_optim=args.resume_optim, val_criterion=val_criterion,
                      logdir=args.logdir, log=log, resident=args.resident_frames)
    trainer.train_val(lstm=False)
    return trainer


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.config_file is None or args.model is None:
        build_parser().error("--config_file and --model are required")
    run(args)


if __name__ == "__main__":
    main()
