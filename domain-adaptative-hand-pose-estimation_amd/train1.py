#!/usr/bin/env python
"""Domain-adaptive hand-pose training on the MI355X kernels — same command line, log / checkpoint layout and
training schedule as the reference's ``train1.py`` (main :37-275, pretrain :278-325, train :328-492,
validate :495-536, CLI :591-675).  Additive flags: ``--synthetic`` (seeded synthetic data instead of the
out-of-scope CPU dataset layer), ``--synthetic-hands`` with ``--render-gap`` / ``--render-train-size`` / ``--render-val-size`` (a rendered
two-domain hand data set drawn on the GPU from per-sample records, with exact key points: utils/rendered_dataset.py), ``--dtype {bf16,f32,fp8,mxfp8}``, ``--mx-eval``, ``--no-graph``, ``--device-augment`` (the training
augmentation chain, the validation resize and the labels of both on the GPU), ``--ema-update {off,const,warmup}`` (keep the
EMA teacher ``model_ema`` up to date: the reference's commented-out call at train1.py:461), ``--mt-loss {off,on}`` with
``--mt-weight`` / ``--mt-k`` (the mean-teacher consistency term on the target batch: the reference's unused ``x_t_ema``, ``m`` and
``mt_loss``, train1.py:351-364 and uda/model/loss.py:265-297), ``--mmd-loss {off,on}`` with ``--mmd-weight`` / ``--mmd-kernels`` /
``--mmd-mul`` (MMD alignment of the target heat-maps with the source heat-maps in step C: the reference's unused ``MMD_loss3``,
uda/model/loss.py:1061-1104), ``--jfa-loss {off,on}`` with ``--jfa-weight`` / ``--jfa-radius`` / ``--jfa-axes`` (alignment of the
neck features pooled around the predicted key points of the target batch with those of the source batch in step C: the
reference's unused ``loss3``, train1.py:25 and uda/model/loss.py:331-378), ``--proto-loss {off,kl,softkl}`` with ``--proto-weight`` /
``--proto-radius`` / ``--proto-axes`` / ``--proto-m`` (alignment of per-joint class prototypes of those features, blended with a running
memory per domain: the reference's unused ``lossx`` / ``lossx3``, uda/model/loss.py:381-466 and 560-652), ``--mixup {off,on}`` with ``--mixup-beta`` / ``--mixup-weight`` /
``--mixup-labels`` (a fourth stage behind update C that trains the backbone and the main head on cross-domain blends of the source
and the target batch, with Gaussian pseudo-labels for the target side: the reference's unused ``mixup``, uda/model/loss.py:13-24), ``--coord-loss {off,source,both}`` with ``--coord-weight`` /
``--coord-target-weight`` / ``--coord-beta`` / ``--coord-delta`` (a coordinate loss on the differentiable soft-arg-max of the source
heat-maps against the un-quantised annotation, and of the target heat-maps against the EMA teacher's: integral regression, not in
the reference), ``--fda {off,on}`` with ``--fda-beta`` (step A sees the source batch with the low-frequency amplitude of the target batch:
Fourier Domain Adaptation, not in the reference), ``--mt-view {same,geom}`` with ``--view-rot`` / ``--view-scale`` / ``--view-shift`` /
``--view-margin`` (the EMA teacher sees the target batch rotated, scaled and shifted per sample and its heat-maps are mapped back
before they are compared: geometric consistency, not in the reference), ``--bone-loss {off,on}`` with ``--bone-weight`` / ``--bone-margin`` / ``--bone-momentum`` / ``--bone-beta`` / ``--bone-eps``
(a bone-ratio skeleton prior on the target prediction against running statistics of the source annotations; not in the reference),
``--occlude {off,keypoint}`` with ``--occlude-p`` / ``--occlude-n`` / ``--occlude-size`` and ``--teacher-conf`` / ``--conf-beta`` (the student sees the
target batch with a patch around key points the EMA teacher is sure of blanked, and the teacher-driven terms leave out the maps
the teacher is not sure of: adaptive occlusion, not in the reference), ``--clip-grad-norm FLOAT``
(global gradient-norm clipping of each of the three updates with a non-finite step guard, on the device; not in the reference), ``--metrics {pck,full}`` with ``--decode {argmax,upsample,quarter,taylor}`` and
``--auc-max-px`` (validation also reports key points in image pixels: end-point error, PCK curve and AUC; the reference's
unused ``compute_uv_from_heatmaps2``, ``accuracy_2d`` and the curve of ``accuracy_3d``, utils/keypoint_detection.py:95-205; the
sub-pixel decodes ``quarter`` and ``taylor`` are not in the reference), ``--flip-test`` with ``--flip-shift`` (validation averages
the heat-maps of every image and its mirror image, as Simple Baselines / HRNet evaluate; not in the reference either).

    python train1.py data/H3D -t Hand3DStudio --synthetic -a resnet50 -b 64

Data parallel (the reference is single-process): start one process per GPU with torchrun,

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 train1.py -- data/H3D ... -b 64

(the ``--`` keeps torchrun's own parser away from the script's flags: ``--log`` is an ambiguous prefix of its ``--log-dir``).

``-b`` stays the per-GPU batch (the path shards by image, BatchNorm statistics stay per GPU as in the reference).  Every
rank reads ``RANK / LOCAL_RANK / WORLD_SIZE`` before touching the GPU, draws its own shard of both training sets
(``DistributedSampler``), the gradient mean of the optimizers about to step is exchanged over RCCL (``mi355.da_step``),
validation counts are summed over ranks, and only rank 0 writes the log and the checkpoints (reference sites made
rank-aware: train1.py:54-99 loaders, :141-154 optimizers, :248-268 checkpoints).
"""
import argparse
import os
import random
import shutil
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch
import torch.distributed as dist
from torch.optim.lr_scheduler import LambdaLR, MultiStepLR
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

import mi355
import uda.model as models
from mi355 import ops as _ops
from mi355.ops import FDA_MAX_B, fda_band
from mi355.da_step import CoordRegression, KinematicPrior, CrossDomainMixup, FourierStyle, JointFeatureAlign, MMDAlign, PrototypeAlign, build_training, broadcast_module, _allreduce_mean
from mi355.optim import EMATeacher, GradClipper, make_optimizer
from mi355.teacher import GeometricView, KeypointOcclusion, MeanTeacher
from uda.model.loss import JointsKLLoss, check_blend_weight, check_positive, check_whole
from uda.model.pose_resnet2 import Upsampling, PoseResNet
from uda.model.regda_7 import MainOutput, PoseResNetx9 as RegDAPoseResNetx1, PoseResNetx10 as RegDAPoseResNetx2
from utils.checkpoint import load_training_state, save_training_state
from utils.data import ForeverDataIterator, DevicePrefetcher, DeviceAugmentIterator, ragged_collate
from utils.keypoint_detection import accuracy, accuracy_from_preds, get_max_preds_device, decode_keypoints, PoseMetrics
from utils.logger import CompleteLogger
from utils.meter import AverageMeter, ProgressMeter, AverageMeterDict

device = torch.device("cuda" if torch.cuda.device_count() > 0 else "cpu")     # device_count() does not initialise the GPU
RANK, WORLD = 0, 1


def init_distributed():
    """One process per GPU: read the torchrun environment BEFORE any GPU call, bind this process to its GPU and join
    the process group (backend nccl = RCCL over xGMI; MI355_DIST_BACKEND=gloo for rehearsals with several ranks on
    one GPU).  Single-process runs (no WORLD_SIZE) skip all of it."""
    global device, RANK, WORLD
    WORLD = int(os.environ.get('WORLD_SIZE', '1'))
    RANK = int(os.environ.get('RANK', '0'))
    if WORLD > 1:
        local = int(os.environ.get('LOCAL_RANK', str(RANK)))
        ndev = torch.cuda.device_count()
        if ndev == 0:
            raise SystemExit('this training path needs an MI355X (HIP kernels only, no CPU fallback)')
        torch.cuda.set_device(local % ndev)
        device = torch.device('cuda', local % ndev)
        if WORLD > ndev:
            # several ranks share a GPU (rehearsal): the one-launch BatchNorm backward wants the whole chip for its resident
            # blocks -- two processes launching it at once would starve each other (include/mi355pose.h, mi355_bn_set_resident)
            os.environ['MI355_BN_RESIDENT'] = '0'
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group(os.environ.get('MI355_DIST_BACKEND', 'nccl'), rank=RANK, world_size=WORLD)
    return RANK, WORLD


def replicas_in_sync(model):
    """Failure detection for the data-parallel run: every rank must hold bit-identical parameters (same initial
    broadcast, same averaged gradients, same deterministic update kernels).  Returns the checksum, raises on drift."""
    cs = torch.stack([p.detach().double().abs().sum() for p in model.parameters()]).sum().reshape(1)
    if WORLD > 1:
        every = [torch.zeros_like(cs) for _ in range(WORLD)]
        dist.all_gather(every, cs)
        if any(float(e) != float(every[0]) for e in every):
            raise RuntimeError('data-parallel replicas diverged: parameter checksums %s' % [float(e) for e in every])
    return float(cs)


RENDERED_LABEL_EPSILON = 1e-12        # JointsKLLoss.epsilon under --synthetic-hands (main(): labels of joints outside the frame)


def build_datasets(args):
    image_size, heatmap_size = (args.image_size,) * 2, (args.heatmap_size,) * 2
    if args.synthetic:
        from utils.synthetic_dataset import SyntheticHand21
        mk = lambda n, seed: SyntheticHand21(n, image_size, heatmap_size, seed=seed)
        n = args.batch_size * max(args.iters_per_epoch, 1)
        return mk(n, 11), mk(4 * args.batch_size, 12), mk(n, 13), mk(4 * args.batch_size, 14)
    if getattr(args, 'synthetic_hands', False):
        # rendered hands: 'cg' source and 'photo' target, both validation sets labelled (as H3D's is), seeds disjoint from training
        from utils.rendered_dataset import RenderedHand21
        mk = lambda n, seed, domain: RenderedHand21(n, image_size, heatmap_size, seed=seed, domain=domain, gap=args.render_gap)
        return (mk(args.render_train_size, 21, 'cg'), mk(args.render_val_size, 22, 'cg'),
                mk(args.render_train_size, 23, 'photo'), mk(args.render_val_size, 24, 'photo'))
    import uda.dataset as datasets                   # RHD / H3D / STB readers + key-point aware augmentation (PIL + numpy)
    import uda.dataset.keypoint_detection as T
    normalize = T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    if args.device_augment:     # same parameters, drawn on the host; the pixel work and the labels run on the GPU
        train_tf = T.DeviceAugment(args.rotation, args.image_size, args.resize_scale)
    else:
        train_tf = T.Compose([T.RandomRotation(args.rotation), T.RandomResizedCrop(size=args.image_size, scale=args.resize_scale),
                              T.ColorJitter(brightness=0.25, contrast=0.25, saturation=0.25), T.GaussianBlur(), T.ToTensor(), normalize])
    if args.device_augment:     # the test sets hand over their sources as well: Resize / ToTensor / Normalize on the GPU
        val_tf = T.DeviceResize(args.image_size)
    else:
        val_tf = T.Compose([T.Resize(args.image_size), T.ToTensor(), normalize])
    src, tgt = datasets.__dict__[args.source], datasets.__dict__[args.target]
    kw = dict(image_size=image_size, heatmap_size=heatmap_size)
    return (src(root=args.source_root, transforms=train_tf, **kw), src(root=args.source_root, split='test', transforms=val_tf, **kw),
            tgt(root=args.target_root, transforms=train_tf, **kw), tgt(root=args.target_root, split='test', transforms=val_tf, **kw))


def make_loader(ds, args, train):
    """train: this rank's shard (reshuffled every pass, ForeverDataIterator advances the sampler epoch); validation: the
    strided shard rank::WORLD without padding, so that the counts summed over ranks are exactly the data set's."""
    # --device-augment: the data sets yield their sources ragged and unprocessed, packed per batch (utils.data.ragged_collate);
    # the validation loaders then only decode, so they get the workers too
    ragged = getattr(args, 'device_augment', False) and not args.synthetic
    collate = ragged_collate if ragged else None
    val_workers = args.workers if ragged else 0
    if getattr(args, 'synthetic_hands', False):          # records, packed per batch (utils.data.record_collate); the GPU draws them
        from utils.data import record_collate
        collate, val_workers = record_collate, args.workers
    if WORLD == 1:
        return DataLoader(ds, batch_size=args.batch_size, shuffle=train, num_workers=args.workers if train else val_workers,
                          pin_memory=True, drop_last=train, collate_fn=collate)
    if train:
        sampler = DistributedSampler(ds, num_replicas=WORLD, rank=RANK, shuffle=True, seed=args.seed or 0, drop_last=True)
        return DataLoader(ds, batch_size=args.batch_size, sampler=sampler, num_workers=args.workers, pin_memory=True, drop_last=True,
                          collate_fn=collate)
    return DataLoader(ds, batch_size=args.batch_size, sampler=list(range(RANK, len(ds), WORLD)), num_workers=val_workers, pin_memory=True,
                      collate_fn=collate)


def main(args):
    init_distributed()
    logger = CompleteLogger(args.log, args.phase, quiet=RANK != 0)      # rank 0 owns the console mirror and the log file
    print(args)
    if device.type != 'cuda':
        raise SystemExit('this training path needs an MI355X (HIP kernels only, no CPU fallback)')
    mi355.load()
    mi355.set_compute_dtype(args.dtype)
    if args.seed is not None:
        random.seed(args.seed + RANK)
        torch.manual_seed(args.seed)             # same initial weights everywhere (and broadcast below anyway)
        warnings.warn('You have chosen to seed training.')
    if WORLD > 1:
        print('data parallel: %d ranks, backend %s, per-GPU batch %d' % (WORLD, dist.get_backend(), args.batch_size))

    train_s, val_s, train_t, val_t = build_datasets(args)
    ld = lambda ds, train: make_loader(ds, args, train)
    train_source_loader, val_source_loader = ld(train_s, True), ld(val_s, False)
    train_target_loader, val_target_loader = ld(train_t, True), ld(val_t, False)
    print("Source train:", len(train_source_loader)); print("Target train:", len(train_target_loader))
    print("Source test:", len(val_source_loader)); print("Target test:", len(val_target_loader))
    train_source_iter, train_target_iter = ForeverDataIterator(train_source_loader), ForeverDataIterator(train_target_loader)
    # who reads the teacher's view of the target batch (meta['image_ema']): the consistency term, and mixup labelled by the teacher
    want_ema = args.mt_loss == 'on' or (args.mixup == 'on' and args.mixup_labels == 'teacher') or args.coord_loss == 'both' or \
        args.occlude == 'keypoint'
    if args.synthetic_hands:
        # records -> HBM, the images (with --mt-loss etc. also the teacher's meta['image_ema']) and the labels on the GPU
        from utils.data import RenderedHandIterator
        rend = lambda it, ema=False, kp=False: RenderedHandIterator(it, device, args.image_size, args.heatmap_size, want_ema=ema,
                                                                    want_keypoints=kp or args.debug)
        train_source_iter, train_target_iter = rend(train_source_iter, kp=wants_keypoints(args)), rend(train_target_iter, want_ema)
    elif args.device_augment and not args.synthetic:
        # packed sources -> HBM, augmentation and heat-map labels on the GPU (mi355.augment, utils.labels)
        dev_aug = lambda it, ema=False: DeviceAugmentIterator(it, device, args.image_size, args.heatmap_size, want_ema=ema)
        # (--mt-loss: the target batches also carry meta['image_ema'], the geometry-only image the teacher sees)
        train_source_iter, train_target_iter = dev_aug(train_source_iter), dev_aug(train_target_iter, want_ema)
    else:
        # host -> HBM copies of the next batch overlap the current step (pinned, double-buffered, side stream)
        # (--mt-loss: meta['image_ema'] of the target batches travels with them instead of as a blocking copy inside the iteration)
        ema_keys = ('image_ema',) if want_ema and not args.synthetic else ()
        # (--coord-loss, --bone-loss: meta['keypoint2d'] of the source batches, the un-quantised key points, travels with them likewise)
        train_source_iter = DevicePrefetcher(train_source_iter, device, meta_keys=('keypoint2d',) if wants_keypoints(args) else ())
        train_target_iter = DevicePrefetcher(train_target_iter, device, meta_keys=ema_keys)

    # model (+ the EMA copy the reference builds and checkpoints, train1.py:102-128; frozen unless --ema-update is on)
    backbone = models.__dict__[args.arch](pretrained=True)
    upsampling = Upsampling(backbone.out_features)
    num_keypoints = train_s.num_keypoints
    model = RegDAPoseResNetx1(backbone, upsampling, 256, num_keypoints, num_head_layers=args.num_head_layers, finetune=True).to(device)
    ema_bb = models.__dict__[args.arch](pretrained=False)
    model_ema = RegDAPoseResNetx2(ema_bb, Upsampling(ema_bb.out_features), 256, num_keypoints,
                                  num_head_layers=args.num_head_layers, finetune=True).to(device)
    for p_main, p_ema in zip(model.parameters(), model_ema.parameters()):
        p_ema.data.copy_(p_main.data)
        p_ema.requires_grad = False

    criterion = JointsKLLoss()
    step, opts, scheds = build_training(model, heatmap_size=args.heatmap_size, lr=args.lr, momentum=args.momentum, wd=args.wd,
                                        lr_gamma=args.lr_gamma, lr_decay=args.lr_decay, trade_off=args.trade_off,
                                        num_keypoints=num_keypoints, optimizer=args.optimizer, adam_betas=tuple(args.adam_betas),
                                        adam_eps=args.adam_eps)
    if args.synthetic or args.synthetic_hands:
        # noise images make the target predictions collapse within a few dozen iterations; the reference's per-map
        # max-normalisation then divides 0 by 0 (regda_7.py:3623-3625).  Synthetic runs keep such maps at zero instead.
        # (rendered hands: an untrained model can still emit an all-zero ground-false map, so the guard stays on)
        for c in step.crit.values():
            if hasattr(c, 'guard_empty_maps'):
                c.guard_empty_maps = True
    if args.synthetic_hands:
        # a rendered joint may lie outside the frame: its label is an all-zero map with weight 0, and the KL loss normalises a label
        # by its sum -- 0 / 0, a NaN that the zero weight does not remove (uda/model/loss.py:145-158; the noise data set keeps every
        # joint in frame).  The loss's own epsilon makes such a label uniform, its row exactly 0; at 1e-12 a labelled map keeps its
        # bits where it is not zero (1 + 1e-12 rounds to 1) and its zero pixels become about 1e-13 of the mass.
        for c in [criterion] + list(step.crit.values()):
            if isinstance(c, JointsKLLoss):
                c.epsilon = RENDERED_LABEL_EPSILON
    ema = None
    if args.ema_update != 'off':
        # the teacher follows the model after every iteration (uda/model/loss.py:252-261 at train1.py:461), on the device
        ema = step.ema = EMATeacher(model, model_ema, opts, args.ema_decay, warmup=args.ema_update == 'warmup')
    # the optional terms of step C's loss (what each adds: the classes' docstrings)
    if args.mt_loss == 'on':
        step.mt = MeanTeacher(ema, weight=args.mt_weight, k=args.mt_k)          # the teacher runs inside the iteration
    if args.mmd_loss == 'on':
        step.mmd = MMDAlign(weight=args.mmd_weight, kernel_mul=args.mmd_mul, kernel_num=args.mmd_kernels)
    if args.jfa_loss == 'on':
        step.jfa = JointFeatureAlign(weight=args.jfa_weight, radius=args.jfa_radius, axes=args.jfa_axes)
    if args.proto_loss != 'off':
        step.proto = PrototypeAlign(weight=args.proto_weight, radius=args.proto_radius, axes=args.proto_axes, m=args.proto_m,
                                    criterion=args.proto_loss)
    if args.mixup == 'on':
        # step M behind update C: blends of the two batches through backbone, neck and main head (mi355.da_step.CrossDomainMixup)
        step.mixup = CrossDomainMixup(beta=args.mixup_beta, weight=args.mixup_weight, labels=args.mixup_labels, ema=ema,
                                      seed=args.seed, rank=RANK)
    if args.mt_view == 'geom':
        # the teacher's forward of the iteration runs on another view of the target batch (mi355.teacher.GeometricView)
        step.view = GeometricView(rot_deg=args.view_rot, scale=tuple(args.view_scale), shift=args.view_shift, margin=args.view_margin,
                                  seed=args.seed, rank=RANK)
    if args.occlude == 'keypoint':
        # the student's forwards of the target batch read it with patches around confident teacher key points blanked
        # (mi355.teacher.KeypointOcclusion); the teacher's forward moves to the head of step B
        step.occlude = KeypointOcclusion(prob=args.occlude_p, n=args.occlude_n, size=tuple(args.occlude_size), beta=args.conf_beta,
                                         seed=args.seed, rank=RANK)
    # a teacher map counts for the teacher-driven terms only when the peak of its softmax reaches --teacher-conf (0: no gate)
    step.teacher_conf, step.conf_beta = float(args.teacher_conf), float(args.conf_beta)
    if args.fda == 'on':
        # step A sees the source batch in the style of the target batch (mi355.da_step.FourierStyle); no state, nothing to checkpoint
        step.fda = FourierStyle(beta=args.fda_beta)
    # step A (and, with 'both', step C against the teacher) gains a loss on the soft-arg-max coordinates
    step.coord = coord_term(args, ema)
    # step A keeps bone-ratio statistics of the source annotations, step C holds the target prediction to them
    step.bone = bone_term(args)
    if args.clip_grad_norm > 0:
        # each update clips the global norm of what it steps and skips itself when that norm is not finite (mi355.optim.GradClipper)
        step.clip = GradClipper(args.clip_grad_norm, device)
    start_epoch = 0
    if args.resume is None:
        if args.pretrain is None or ((args.synthetic or args.synthetic_hands) and not os.path.exists(args.pretrain)):
            print("Pretraining the model on source domain.")
            args.pretrain = logger.get_checkpoint_path('pretrain')
            pre = PoseResNet(backbone, upsampling, 256, num_keypoints, True).to(device)
            optimizer = make_optimizer(args.optimizer, pre.get_parameters(lr=args.lr), lr=args.lr, momentum=args.momentum,
                                       weight_decay=args.wd, betas=tuple(args.adam_betas), eps=args.adam_eps)
            lr_scheduler = MultiStepLR(optimizer, args.lr_step, args.lr_factor)
            best_acc = -1
            pre_clip = GradClipper(args.clip_grad_norm, device) if args.clip_grad_norm > 0 else None
            for epoch in range(args.pretrain_epochs):
                lr_scheduler.step()                      # the reference steps the schedule before the epoch (train1.py:167)
                pretrain(train_source_iter, pre, criterion, optimizer, epoch, args, clip=pre_clip)
                acc = validate(val_source_loader, pre, criterion, args)
                _ops.bn_resident_check('pre-training epoch %d' % epoch)   # (validation has synchronised: the poll is free)
                if acc['all'] > best_acc:
                    best_acc = acc['all']
                    if RANK == 0:
                        torch.save({'model': pre.state_dict()}, args.pretrain)
                print("Source: {} best: {}".format(acc['all'], best_acc))
            if WORLD > 1:
                dist.barrier()                           # rank 0 has written the file everybody reads next
        pretrained_dict = torch.load(args.pretrain, map_location='cpu', weights_only=False)['model']
        model_dict = model.state_dict()
        pretrained_dict = {k: v for k, v in pretrained_dict.items() if k in model_dict}
        model.load_state_dict(pretrained_dict, strict=False)
        model_ema.load_state_dict(pretrained_dict, strict=False)
    else:
        start_epoch = load_training_state(args.resume, args, model, model_ema, opts, scheds, step, ema, device)
    broadcast_module(model)                              # replicas start bit-identical whatever each rank loaded
    broadcast_module(model_ema)

    if args.phase == 'test':
        s_acc = validate(val_source_loader, model, criterion, args)
        t_acc = validate(val_target_loader, model, criterion, args)
        print("Source: {:4.3f} Target: {:4.3f}".format(s_acc['all'], t_acc['all']))
        for name, acc in t_acc.items():
            print("{}: {:4.3f}".format(name, acc))
        logger.close()
        return

    best_acc = 0
    print("Start regression domain adaptation.")
    for epoch in range(start_epoch, args.epochs):
        logger.set_epoch(epoch)
        print(*[scheds[k].get_last_lr() for k in ('f', 'h', 'h_adv', 'h_adv2')])
        train(train_source_iter, train_target_iter, step, scheds, epoch, args, logger=logger)
        if step.clip is not None:
            print('skipped steps: %d' % step.clip.read()[1])       # (a count since the start of this process: not checkpointed)
        s_acc = validate(val_source_loader, model, criterion, args)
        t_acc = validate(val_target_loader, model, criterion, args)
        e_acc = validate(val_target_loader, MainOutput(model_ema), criterion, args) if ema is not None else None   # (validate2, :243)
        # a one-launch BatchNorm backward whose blocks could not all get onto the chip has written NaN gradients: raise
        # instead of training on (the poll synchronises, validation just has)
        step.check_health('epoch %d' % epoch)
        if WORLD > 1:
            print('replicas in sync (parameter checksum %.6e)' % replicas_in_sync(model))
        if RANK != 0:
            if WORLD > 1:
                dist.barrier()
            best_acc = max(best_acc, t_acc['all'])
            continue
        save_training_state(logger.get_checkpoint_path(epoch), epoch, args, model, model_ema, opts, scheds, step, ema)
        if t_acc['all'] > best_acc:
            shutil.copy(logger.get_checkpoint_path(epoch), logger.get_checkpoint_path('best'))
            best_acc = t_acc['all']
        if WORLD > 1:
            dist.barrier()                               # checkpoints of this epoch are complete
        print("Source: {:4.3f} Target: {:4.3f} Target(best): {:4.3f}".format(s_acc['all'], t_acc['all'], best_acc))
        if e_acc is not None:
            print("ema: {:4.3f}".format(e_acc['all']))
        for name, acc in t_acc.items():
            print("{}: {:4.3f}".format(name, acc))
    logger.close()
    if WORLD > 1:
        dist.destroy_process_group()


def pretrain(train_source_iter, model, criterion, optimizer, epoch, args, clip=None):
    batch_time, data_time = AverageMeter('Time', ':4.2f'), AverageMeter('Data', ':3.1f')
    losses_s, acc_s = AverageMeter('Loss (s)', ":.2e"), AverageMeter("Acc (s)", ":3.2f")
    progress = ProgressMeter(args.iters_per_epoch, [batch_time, data_time, losses_s, acc_s], prefix="Epoch: [{}]".format(epoch))
    model.train()
    end = time.time()
    for i in range(args.iters_per_epoch):
        optimizer.zero_grad()
        x_s, label_s, weight_s, _ = next(train_source_iter)
        x_s, label_s, weight_s = x_s.to(device, non_blocking=True), label_s.to(device, non_blocking=True), weight_s.to(device, non_blocking=True)
        data_time.update(time.time() - end)
        y_s = model(x_s)
        loss_s = criterion(y_s, label_s, weight_s)
        loss_s.backward()
        if WORLD > 1:
            _allreduce_mean(optimizer.flat_grads())     # gradient mean over ranks (the flat buffers are the buckets)
        if clip is None:
            optimizer.step()
        else:
            optimizer.step(clip=clip.measure([optimizer], 'a'))
        if i % args.print_freq == 0:                    # host reads only when something is printed
            _, avg_acc_s, cnt_s, _ = accuracy(y_s.detach(), label_s)
            acc_s.update(avg_acc_s, cnt_s); losses_s.update(float(loss_s), cnt_s)
            batch_time.update(time.time() - end)
            progress.display(i)
        end = time.time()


def _pck(dists, thr=0.5):
    """avg accuracy + count from a (B,K) device tensor of PCK distances (-1 = ignored), utils/keypoint_detection.py:53-92."""
    d = dists.t().cpu().numpy()
    accs = [float((row[row != -1] < thr).mean()) for row in d if (row != -1).any()]
    return (sum(accs) / len(accs) if accs else 0), len(accs)


def coord_term(args, ema):
    """The ``mi355.da_step.CoordRegression`` of --coord-loss source|both; None when the switch is off."""
    if args.coord_loss == 'off':
        return None
    return CoordRegression(weight=args.coord_weight, beta=args.coord_beta, delta=args.coord_delta,
                           target='teacher' if args.coord_loss == 'both' else 'off', target_weight=args.coord_target_weight, ema=ema)


def bone_term(args):
    """The ``mi355.da_step.KinematicPrior`` of --bone-loss on; None when the switch is off."""
    if args.bone_loss == 'off':
        return None
    return KinematicPrior(weight=args.bone_weight, margin=args.bone_margin, momentum=args.bone_momentum, beta=args.bone_beta,
                          eps=args.bone_eps)


def wants_keypoints(args):
    """Does some term read batch['kp_s'], the un-quantised source key points?"""
    return args.coord_loss != 'off' or args.bone_loss == 'on'


def source_keypoints(meta, image_size, heatmap_size, device):
    """batch['kp_s']: ``meta['keypoint2d']`` (B, K, 2) in image pixels -> fp32 heat-map pixels on `device`, un-quantised (the labels
    sit at ``int(. + 0.5)`` of these)."""
    kp = torch.as_tensor(meta['keypoint2d']).to(device, non_blocking=True)
    return (kp.float() / (float(image_size) / float(heatmap_size))).contiguous()


def train(train_source_iter, train_target_iter, step, scheds, epoch, args, logger=None):
    names = ['Time', 'Data', 'Loss (s)', 'Loss (t, false)', 'Loss (t, truth)', 'Acc (s)', 'Acc (t)', 'Acc (s, adv)', 'Acc (t, adv)']
    fmts = [':4.2f', ':3.1f', ':.2e', ':.2e', ':.2e', ':3.2f', ':3.2f', ':3.2f', ':3.2f']
    mt, terms, mixup, coord = step.mt, step.terms(), step.mixup, step.coord
    if mt is not None:
        mt.set_epoch(epoch)                              # m and k are functions of the epoch (train1.py:351-353)
    keys = (['coord'] if coord is not None else []) + [t.key for t in terms] + (['mix'] if mixup is not None else [])
    names, fmts = names + ['Loss (%s)' % k for k in keys], fmts + [':.2e'] * len(keys)
    # device scalars of the occlusion and the confidence gate: mean boxes per sample, share of confident teacher maps
    occluding = getattr(step, 'occlude', None) is not None and step.occlude.n > 0
    gauges = ([('Occl', 'occ_boxes')] if occluding else []) + ([('Conf', 'conf_share')] if occluding or getattr(step, 'teacher_conf', 0.0) > 0 else [])
    names, fmts = names + [n for n, _ in gauges], fmts + [':4.2f'] * len(gauges)
    clip, n_fixed = step.clip, 9 + len(keys) + len(gauges)
    if clip is not None:                                 # the gradient norms of the updates, read when a line is printed
        if mixup is not None:
            clip.ensure_slot('m')                        # update M's record
        names, fmts = names + ['GradNorm (%s)' % s.upper() for s in clip.SLOTS], fmts + [':.2e'] * len(clip.SLOTS)
    meters = [AverageMeter(n, f) for n, f in zip(names, fmts)]
    progress = ProgressMeter(args.iters_per_epoch, meters, prefix="Epoch: [{}]".format(epoch))
    end = time.time()
    for i in range(args.iters_per_epoch):
        x_s, label_s, weight_s, meta_s = next(train_source_iter)
        x_t, label_t, weight_t, meta_t = next(train_target_iter)
        to = lambda t: t.to(device, non_blocking=True)
        batch = dict(x_s=to(x_s), label_s=to(label_s), w_s=to(weight_s), x_t=to(x_t), w_t=to(weight_t), label_t=to(label_t))
        if coord is not None or getattr(step, 'bone', None) is not None:   # the un-quantised source key points, image pixels -> heat-map pixels
            batch['kp_s'] = source_keypoints(meta_s, args.image_size, args.heatmap_size, device)
        if mt is not None or (mixup is not None and mixup.labels == 'teacher') or (coord is not None and coord.target == 'teacher') or occluding:   # x_t_ema = meta_t['image_ema'] (train1.py:364); synthetic images have no augmentation
            batch['x_t_ema'] = batch['x_t'] if args.synthetic else to(meta_t['image_ema'])
        meters[1].update(time.time() - end)
        # HIP-graph replay once this process has run three eager iterations (whatever epoch it resumed at).  With several
        # ranks the eager path overlaps the gradient exchange with the backward, which only pays while the host can enqueue an
        # iteration faster than the GPU runs it: the fourth iteration is timed on host and GPU and every rank takes the same
        # decision (DAStep.choose_launch_mode, the rule bench.py uses; MI355_DDP_GRAPH=1 / 0 forces it)
        step.eager_iters = getattr(step, 'eager_iters', 0)
        if step.graphs is None and not args.no_graph and step.eager_iters == 3 and not getattr(step, 'mode_chosen', False):
            step.mode_chosen = True
            mode = 'graph'
            if WORLD > 1:
                mode = step.choose_launch_mode(batch, after=lambda: [s.step() for s in scheds.values()])
                print('multi-rank launch mode: host / GPU time of an eager iteration %.2f -> %s'
                      % (step.host_gpu_ratio, ('HIP-graph replay, overlapped RCCL gradient exchange captured with the graphs' if step._overlap_capturable()
                                                 else 'HIP-graph replay, collectives between the graphs') if mode == 'graph'
                         else 'eager launches, gradient exchange overlapped with the backward'))
                step.eager_iters += 1
                end = time.time()
                if mode == 'graph':
                    step.capture(batch, warmup=0)
                continue                                      # (the timed iteration was a real one)
            step.capture(batch, warmup=0)
            print('HIP graphs captured: iterations replay %s graphs from here on' % ('six' if len(step.graphs) == 6 else len(step.graphs)))
        elif step.graphs is None and step.eager_iters == 0:
            print('eager kernel launches%s' % (' with the gradient exchange overlapped with the backward' if WORLD > 1 else ''))
        step.eager_iters += 1
        out = step.run(batch)                            # steps A, B, C + GL step (train1.py:371-453)
        for s in scheds.values():
            s.step()
        if i % args.print_freq == 0:
            for m, k in zip(meters[2:5], ('loss_s', 'loss_gf', 'loss_gt')):
                m.update(float(out[k]), args.batch_size)
            for m, k in zip(meters[5:9], ('pck_s', 'pck_t', 'pck_s_adv', 'pck_t_adv')):
                a, c = _pck(out[k]); m.update(a, c)
            for m, k in zip(meters[9:], keys):
                m.update(float(out['loss_' + k]), args.batch_size)
            for m, (_, k) in zip(meters[9 + len(keys):], gauges):
                if k in out:                             # (conf_share appears with the first teacher forward that is gated)
                    m.update(float(out[k]), args.batch_size)
            if clip is not None:
                norms = clip.read()[0]
                for m, s in zip(meters[n_fixed:], clip.SLOTS):
                    m.update(norms[s][0], 1)
            meters[0].update(time.time() - end)
            progress.display(i)
            if args.debug and getattr(args, 'synthetic_hands', False) and logger is not None and RANK == 0:
                debug_images(batch, out, meta_s, meta_t, logger, i)      # (outside the captured graphs; one device read)
        end = time.time()


def debug_images(batch, out, meta_s, meta_t, logger, i):
    """--debug under --synthetic-hands: sample 0 of the source and of the target batch, de-normalised, with the predicted (red) and
    the labelled (green) skeleton, written to the logger's visualize/ directory.  Everything needed travels in one device read."""
    from utils.visualize import visualize
    S, K = batch['x_s'].shape[-1], out['y_s'].shape[1]
    parts = []
    for x, y, meta in ((batch['x_s'], out['y_s'], meta_s), (batch['x_t'], out['y_t'], meta_t)):
        pred = get_max_preds_device(y[:1])[0].reshape(-1).float() * (float(S) / float(y.shape[-1]))
        parts += [x[0].reshape(-1).float(), pred, meta['keypoint2d'][0].reshape(-1).float()]
    flat = torch.cat(parts).cpu().numpy()
    n, o = 3 * S * S, 0
    for name in ('source', 'target'):
        image, pred, label = flat[o:o + n].reshape(3, S, S), flat[o + n:o + n + 2 * K].reshape(K, 2), flat[o + n + 2 * K:o + n + 4 * K].reshape(K, 2)
        visualize(image, pred, label, logger.get_image_path('%s_%d.jpg' % (name, i)))
        o += n + 4 * K


def validate_batch_metrics(y, label, weight, criterion):
    """The per-batch metric step of validate(): (0-d loss, predicted (B,K,2) and labelled (B,K,2) heat-map maxima), all on the
    device -- three launches and no host synchronisation."""
    return criterion(y, label, weight).detach(), get_max_preds_device(y)[0], get_max_preds_device(label)[0]


def _allreduce_sum(t):
    if WORLD > 1:
        dist.all_reduce(t)


def validate(val_loader, model, criterion, args, dump=None):
    """The host reads the metrics only when a progress line is due and at the end, so the printed Time field is the mean over
    the batches since the last read (time since then / batches metered), not the time of the single last batch.

    ``--metrics full``: every batch is also decoded to image pixels (``--decode``) and added to a PoseMetrics against
    ``meta['keypoint2d']`` with ``weight`` as visibility -- launches only, nothing is read per batch; one more line (EPE, AUC)
    and the per-group EPEs are printed at the end.  ``dump`` (a dict, test.py --dump-preds): filled with the predictions of the
    whole data set in data-set order (rank 0; None elsewhere) and the reported numbers.

    ``--flip-test``: every batch goes through the network together with its mirror image (FlipForward: one forward of twice the
    batch) and the two sets of heat-maps are averaged (``--flip-shift``); the loss, the heat-map PCK and the ``--metrics full``
    decode all use the average.  With ``--metrics full`` the average comes out of the decode's own launch."""
    full = getattr(args, 'metrics', 'pck') == 'full'
    flip, shift = bool(getattr(args, 'flip_test', False)), int(getattr(args, 'flip_shift', 1))
    mode = getattr(args, 'decode', 'argmax')
    batch_time, losses = AverageMeter('Time', ':6.3f'), AverageMeter('Loss', ':.2e')
    dataset = val_loader.dataset
    acc = AverageMeterDict(dataset.keypoints_group.keys(), ":3.2f")
    progress = ProgressMeter(len(val_loader), [batch_time, losses, acc['all']], prefix='Test: ')
    model.eval()
    if getattr(args, 'mx_eval', False):
        mi355.set_mx_eval(True)              # (eval-mode modules only: training forwards are not affected)
    from mi355.infer import FlipForward, GraphedForward
    forward = (FlipForward if flip else GraphedForward)(model)   # full batches replay one HIP graph; the ragged last batch runs eagerly
    sigma = getattr(args, 'decode_sigma', None)
    if sigma is None:
        sigma = getattr(dataset, 'sigma', 2.0)
    batches = val_loader
    if getattr(getattr(dataset, 'transforms', None), 'labels_on_device', False):
        # DeviceResize data set: packed sources -> HBM, resize + normalisation and the heat-map labels on the GPU
        batches = DeviceAugmentIterator(val_loader, device, dataset.image_size[0], dataset.heatmap_size[0], dataset.sigma,
                                        geometry_only=True)
    if getattr(dataset, 'records_on_device', False):
        # RenderedHand21: records -> HBM, the images and the heat-map labels on the GPU; meta['keypoint2d'] is the model's own joints
        from utils.data import RenderedHandIterator
        batches = RenderedHandIterator(val_loader, device, dataset.image_size[0], dataset.heatmap_size[0], dataset.sigma,
                                       want_keypoints=True)
    pending = []                             # (loss, pred, label pred, batch size, heat-map h, w) of the batches not yet metered
    pose = PoseMetrics(dataset.num_keypoints, args.auc_max_px, device=device) if full else None
    kept = []                                # --dump-preds: (pred, gt, visible, maxval) of every batch, on the device

    def meter(since):
        # one stack and one copy per kind, then the meters replayed batch by batch (reference arithmetic, train1.py:505-524)
        if not pending:
            return
        loss_h = torch.stack([p[0] for p in pending]).cpu().tolist()
        pred_h = torch.cat([p[1] for p in pending]).cpu().numpy()
        tgt_h = torch.cat([p[2] for p in pending]).cpu().numpy()
        per_batch, o = (time.time() - since) / len(pending), 0
        for (_, _, _, n, h, w), loss_i in zip(pending, loss_h):
            losses.update(loss_i, n)
            acc.update(dataset.group_accuracy(accuracy_from_preds(pred_h[o:o + n], tgt_h[o:o + n], h, w)[0]), n)
            batch_time.update(per_batch)
            o += n
        pending.clear()

    with torch.no_grad():
        end = time.time()
        for i, (x, label, weight, meta) in enumerate(batches):
            x, label, weight = x.to(device, non_blocking=True), label.to(device, non_blocking=True), weight.to(device, non_blocking=True)
            if flip:
                y, y_flip = forward(x)
                if full:
                    kp, mv, y = decode_keypoints(y, x.shape[3], mode, with_maxval=True, y_flip=y_flip, flip_shift=shift, sigma=sigma,
                                                 return_avg=True)
                else:
                    y = _ops.flip_decode(y, y_flip, shift, want_avg=True)[3]
            else:
                y = forward(x)
            pending.append(validate_batch_metrics(y, label, weight, criterion) + (x.size(0), y.shape[2], y.shape[3]))
            if full:
                if not flip:
                    kp, mv = decode_keypoints(y, x.shape[3], mode, with_maxval=True, sigma=sigma)
                gt = torch.as_tensor(meta['keypoint2d']).float().to(device, non_blocking=True)
                vis = weight.reshape(gt.shape[0], -1)
                pose.update(kp, gt, vis)
                if dump is not None:
                    kept.append((kp, gt, vis, mv.reshape(vis.shape)))
            if i % args.print_freq == 0:     # the host reads only when something is printed, and once at the end
                meter(end)
                end = time.time()
                progress.display(i)
        meter(end)
    if WORLD > 1:                                        # sums and counts over all shards (train1.py:505-524 per shard)
        keys = list(acc.dict.keys())
        t = torch.tensor([v for k in keys for v in (acc[k].sum, acc[k].count)] + [losses.sum, losses.count],
                         dtype=torch.float64, device=device)
        dist.all_reduce(t)
        t = t.cpu().tolist()
        for j, k in enumerate(keys):
            acc[k].sum, acc[k].count = t[2 * j], t[2 * j + 1]
            acc[k].avg = acc[k].sum / max(acc[k].count, 1)
    if full:
        res = pose.result(dataset.keypoints_group, reduce=_allreduce_sum)
        print('EPE: {:.3f} px  AUC(0-{:g}px): {:.4f}'.format(res['epe'], args.auc_max_px, res['auc']))
        for name in dataset.keypoints_group:
            print('EPE {}: {:.3f} px'.format(name, res['epe_' + name]))
        if dump is not None:
            dump.update(_gather_preds(kept, len(dataset), dataset.num_keypoints), image_size=x.shape[3], decode=mode, flip_test=flip, flip_shift=shift,
                        thresholds=res['thresholds'], epe=res['epe'], auc=res['auc'], pck_curve=res['pck_curve'])
    return acc.average()


def _gather_preds(kept, n_total, K):
    """The per-batch (pred, gt, visible, maxval) device tensors of this rank's shard (rank::WORLD, make_loader) -> numpy arrays
    of the whole data set in data-set order on rank 0 (None elsewhere): one concatenation and one copy per split."""
    names = ('pred', 'gt', 'visible', 'maxval')
    if kept:
        flat = torch.cat([torch.cat([t.reshape(t.shape[0], -1).float() for t in row], 1) for row in kept])      # (n, 6K)
    else:
        flat = torch.zeros((0, 6 * K), dtype=torch.float32, device=device)
    if WORLD > 1:
        per = (n_total + WORLD - 1) // WORLD                 # the longest shard; shorter ones are padded for the gather
        pad = torch.zeros((per, 6 * K), dtype=torch.float32, device=device)
        pad[:flat.shape[0]] = flat
        every = [torch.zeros_like(pad) for _ in range(WORLD)]
        dist.all_gather(every, pad)
        if RANK != 0:
            return {k: None for k in names}
        full = torch.zeros((n_total, 6 * K), dtype=torch.float32, device=device)
        for r, part in enumerate(every):
            full[r::WORLD] = part[:len(range(r, n_total, WORLD))]
        flat = full
    a = flat.cpu().numpy()
    return {'pred': a[:, :2 * K].reshape(-1, K, 2), 'gt': a[:, 2 * K:4 * K].reshape(-1, K, 2), 'visible': a[:, 4 * K:5 * K],
            'maxval': a[:, 5 * K:]}


# (flags, kwargs) for every option of the reference's command line (train1.py:602-674: same names, types and
# defaults), followed by the additive ones of this implementation
def _mt_weight(text):
    return 'ref' if text == 'ref' else float(text)


def _clip_norm(text):
    v = float(text)
    if not v >= 0:                                       # (NaN fails the comparison too)
        raise argparse.ArgumentTypeError('a gradient norm cannot be %s: 0 (off), a positive number or inf' % text)
    return v


_OPTIONS = [
    (('--source_root',), dict(default='data/RHD', help='source dataset directory')),
    (('target_root',), dict(help='target dataset directory')),
    (('-s', '--source'), dict(default='RenderedHandPose', help='source dataset class')),
    (('-t', '--target'), dict(help='target dataset class')),
    (('--resize-scale',), dict(nargs='+', type=float, default=(0.6, 1.3), help='RandomResizedCrop scale range')),
    (('--rotation',), dict(type=int, default=180, help='RandomRotation range in degrees')),
    (('--image-size',), dict(type=int, default=256, help='network input side')),
    (('--heatmap-size',), dict(type=int, default=64, help='heat-map side of the main head')),
    (('-a2', '--arch2'), dict(metavar='ARCH', default='net_hg', help='unused (reference CLI parity)')),
    (('--pretrain',), dict(type=str, default='models/pretrain_rhd.pth', help='source-only pre-training checkpoint')),
    (('--ema_model',), dict(type=str, default=None, help='checkpoint whose `model_ema` key holds the EMA teacher: read on '
                          '--resume when --ema-update is on (train1.py), evaluated in addition to --checkpoint (test.py)')),
    (('--resume',), dict(type=str, default=None, help='checkpoint to continue from')),
    (('--resume2',), dict(type=str, default=None, help='unused (reference CLI parity)')),
    (('--num-head-layers',), dict(type=int, default=2)),
    (('--margin',), dict(type=float, default=4., help='unused (reference CLI parity)')),
    (('--trade-off',), dict(default=1., type=float, help='weight of the target-domain disparity losses')),
    (('-b', '--batch-size'), dict(default=32, type=int, metavar='N', help='images per domain per iteration')),
    (('--lr', '--learning-rate'), dict(default=0.01, type=float, metavar='LR', dest='lr', help='base learning rate')),
    (('--momentum',), dict(default=0.9, type=float, metavar='M', help='SGD momentum (ignored with --optimizer adam | adamw)')),
    (('--wd', '--weight-decay'), dict(default=0.0001, type=float, metavar='W')),
    (('--lr-gamma',), dict(default=0.0001, type=float, help='inverse-decay schedule: lr * (1 + gamma * it) ** -decay')),
    (('--lr-decay',), dict(default=0.75, type=float)),
    (('--lr-step',), dict(default=[45, 60], type=tuple, help='pre-training MultiStepLR milestones')),
    (('--lr-factor',), dict(default=0.1, type=float, help='pre-training MultiStepLR factor')),
    (('-j', '--workers'), dict(default=4, type=int, metavar='N', help='loader worker processes')),
    (('--pretrain_epochs',), dict(default=70, type=int, metavar='N')),
    (('--epochs',), dict(default=200, type=int, metavar='N')),
    (('-i', '--iters-per-epoch'), dict(default=500, type=int)),
    (('-p', '--print-freq'), dict(default=100, type=int, metavar='N')),
    (('--seed',), dict(default=1, type=int)),
    (('--log',), dict(type=str, default='logs/mt', help='run directory (logs, checkpoints, images)')),
    (('--phase',), dict(type=str, default='train', choices=['train', 'test'])),
    (('--debug',), dict(action='store_true', help='with --synthetic-hands: at every print interval, write sample 0 of the source and of '
                       'the target batch with the predicted and the labelled skeleton to <log>/visualize/<epoch>/; otherwise accepted '
                       'for CLI parity and ignored')),
    (('--ema-decay',), dict(default=0.999, type=float, metavar='ALPHA', help='decay m of the EMA teacher (--ema-update): v_ema = v_ema * m + (1 - m) * v')),
    # additive
    (('--synthetic',), dict(action='store_true', help='seeded synthetic batches instead of the CPU dataset layer')),
    (('--synthetic-hands',), dict(action='store_true', help="a rendered two-domain hand data set instead of the data sets on disk "
                                 "(utils/rendered_dataset.py): a procedural articulated hand drawn on the GPU from per-sample records, "
                                 "'cg' renders as the source and 'photo' renders (cluttered background, occluder, sensor noise, colour "
                                 "jitter) as the target, both with exact key points; the data roots are ignored, as under --synthetic, "
                                 "which it excludes")),
    (('--render-gap',), dict(default=1.0, type=float, metavar='FLOAT', help="--synthetic-hands: how far the 'photo' distributions lie from the "
                            "'cg' ones, 0 (the same distribution) .. 1 (the full gap)")),
    (('--render-train-size',), dict(default=65536, type=int, metavar='N', help='--synthetic-hands: training items per domain')),
    (('--render-val-size',), dict(default=512, type=int, metavar='N', help='--synthetic-hands: validation items per domain (seeds '
                                 'disjoint from the training sets)')),
    (('--dtype',), dict(default='bf16', choices=['bf16', 'f32', 'fp8', 'mxfp8'], help="compute dtype of activations / packed weights ('fp8': bf16 storage, fp8 operands in the K-heavy conv GEMMs; 'mxfp8': the same convs and the neck's transposed convs on block-scaled MX e4m3 operands)")),
    (('--mx-eval',), dict(action='store_true', help='validation / test forwards: the BatchNorm-folded 3x3 / 4x4 convs and transposed convs '
                          'on block-scaled MX e4m3 operands (opt-in, any --dtype with bf16 activations; also MI355_MX_EVAL=1)')),
    (('--ema-update',), dict(default='off', choices=['off', 'const', 'warmup'], help="update the EMA teacher after every iteration on the "
                            "GPU, validate it on the target set ('ema:' line) and checkpoint it (model_ema.pth, ema_state): 'const' uses "
                            "--ema-decay, 'warmup' min(1 - 1/(step + 1), --ema-decay); 'off': the teacher stays at its initial weights")),
    (('--mt-loss',), dict(default='off', choices=['off', 'on'], help="mean-teacher consistency on the target batch: step C's loss gains "
                         "m * mt_loss(y_t, model_ema(x_t_ema), weight_t, k), the teacher running in eval mode inside the iteration; needs "
                         "--ema-update const|warmup")),
    (('--mt-weight',), dict(default='ref', type=_mt_weight, metavar='ref|FLOAT', help="weight m of the consistency term: 'ref' is the "
                           "reference schedule (0.01 * epoch, 0.3 once epoch > 30), a number a constant")),
    (('--mt-k',), dict(default='all', choices=['all', 'epoch'], help="joints the consistency term compares: 'all' (k = 400) or the "
                      "reference's curriculum with k = epoch (the wrist below 100, one more joint per finger every 100 epochs)")),
    (('--mmd-loss',), dict(default='off', choices=['off', 'on'], help="MMD alignment of the target heat-maps with the source heat-maps: "
                          "step C's loss gains w * MMD_loss3(y_s.detach(), y_t), the per-joint multi-Gaussian-kernel MMD of "
                          "uda/model/loss.py:1061-1104, computed by the mmd_ kernels; 'off': nothing is launched")),
    (('--mmd-weight',), dict(default=0.1, type=float, metavar='FLOAT', help='weight w of the MMD term (constant, positive)')),
    (('--mmd-kernels',), dict(default=5, type=int, metavar='N', help='Gaussian kernels of the MMD term (1 .. 8)')),
    (('--mmd-mul',), dict(default=2.0, type=float, metavar='FLOAT', help='ratio of successive kernel bandwidths of the MMD term')),
    (('--jfa-loss',), dict(default='off', choices=['off', 'on'], help="joint feature alignment: step C's loss gains "
                          "w * loss3(f_t, <source descriptors>, xy_t, .), the KL divergence between the channel distributions of the neck "
                          "features pooled around the predicted key points of the target and of the source batch "
                          "(uda/model/loss.py:331-378), computed by the jfa_ kernels; 'off': nothing is launched")),
    (('--jfa-weight',), dict(default=1.0, type=float, metavar='FLOAT', help='weight w of the joint feature alignment term (constant, '
                            'positive; the default is a placeholder: its effect on convergence has not been measured)')),
    (('--jfa-radius',), dict(default=6, type=int, metavar='N', help='half side of the pooling window in heat-map pixels (1 .. 16)')),
    (('--jfa-axes',), dict(default='xy', choices=['xy', 'ref'], help="'xy': y selects the rows of the feature map; 'ref': the "
                          "reference's indexing, x selects the rows (uda/model/loss.py:353)")),
    (('--proto-loss',), dict(default='off', choices=['off', 'kl', 'softkl'], help="prototype alignment with running memory: step C's "
                            "loss gains w * lossx ('kl', uda/model/loss.py:381-466) or w * lossx3 ('softkl', :560-652) between the per-joint "
                            "class prototypes of the target and of the source batch -- the neck features pooled around the predicted "
                            "key points, averaged over the batch and blended with a memory per domain -- computed by the proto_ "
                            "kernels; the memories travel in the epoch checkpoint (proto_state); 'off': nothing is launched")),
    (('--proto-weight',), dict(default=1.0, type=float, metavar='FLOAT', help='weight w of the prototype alignment term (constant, '
                              'positive; the default is a placeholder: its effect on convergence has not been measured)')),
    (('--proto-radius',), dict(default=6, type=int, metavar='N', help='half side of the pooling window in heat-map pixels (1 .. 16)')),
    (('--proto-axes',), dict(default='xy', choices=['xy', 'ref'], help="'xy': y selects the rows of the feature map; 'ref': the "
                            "reference's indexing, x selects the rows (uda/model/loss.py:421)")),
    (('--proto-m',), dict(default=0.999, type=float, metavar='FLOAT', help="weight m of the current batch in the prototype, the memory "
                         "gets 1 - m (0 < m <= 1; 0.999 is the reference's constant, uda/model/loss.py:400)")),
    (('--mixup',), dict(default='off', choices=['off', 'on'], help="cross-domain mixup: a fourth stage (step M) behind update C blends "
                       "every source image with the target image of the same index by max(l, 1 - l), l ~ Beta(b, b), the heat-map "
                       "labels likewise -- the reference's unused mixup, uda/model/loss.py:13-24, as one mixup_ kernel launch -- and "
                       "trains the backbone, the neck and the main head on the 2 B blends with w * KL (one more forward and backward, "
                       "then update M of optimizer_f and optimizer_h; the EMA update moves behind it); the target side is labelled "
                       "with Gaussians at the arg-max of a prediction (--mixup-labels); the coefficients come from an RNG state of "
                       "their own, seeded from --seed and the rank, kept in the epoch checkpoint (mixup_state); 'off': nothing is "
                       "launched")),
    (('--mixup-beta',), dict(default=1.0, type=float, metavar='FLOAT', help='concentration b of the Beta(b, b) the blend coefficients '
                            'are drawn from (positive; the default is a placeholder: its effect on convergence has not been measured, '
                            'and cannot be without the data sets)')),
    (('--mixup-weight',), dict(default=1.0, type=float, metavar='FLOAT', help='weight w of the mixup loss (constant, positive; the '
                              'default is a placeholder: its effect on convergence has not been measured, and cannot be without the '
                              'data sets)')),
    (('--mixup-labels',), dict(default='student', choices=['student', 'teacher'], help="whose prediction on the target batch labels "
                              "it for --mixup: 'student' = the model's own y_t of step C; 'teacher' = the EMA teacher's on its view of "
                              "the target batch (needs --ema-update const|warmup; with --mt-loss on the teacher's forward of step C "
                              "is reused)")),
    (('--mt-view',), dict(default='same', choices=['same', 'geom'], help="what the EMA teacher sees of the target batch: 'same' = the "
                         "loader's geometry (x_t_ema differs from x_t by colour jitter and blur only); 'geom' = per sample another "
                         "rotation, scale and shift (--view-rot / --view-scale / --view-shift), its heat-maps mapped back to the "
                         "loader's frame before --mt-loss on, --coord-loss both and --mixup-labels teacher read them, and the maps "
                         "whose peak the teacher did not see --view-margin pixels inside its frame left out of all three (Kim et "
                         "al., ECCV 2022; not in the reference); two kernel launches around the teacher's forward, forward only; the "
                         "views come from an RNG state of their own, seeded from --seed and the rank, kept in the epoch checkpoint "
                         "(view_state); needs --ema-update const|warmup and one of the three consumers; 'same': nothing is launched")),
    (('--view-rot',), dict(default=30.0, type=float, metavar='DEG', help='--mt-view geom: the angle is drawn from U(-DEG, DEG) (0 .. 180; '
                          'the default is a placeholder: its effect on convergence has not been measured, and cannot be without the '
                          'data sets)')),
    (('--view-scale',), dict(default=[0.75, 1.25], type=float, nargs=2, metavar=('LO', 'HI'), help='--mt-view geom: the scale is drawn '
                            'from U(LO, HI) (0 < LO <= HI; the defaults are placeholders: their effect on convergence has not been '
                            'measured, and cannot be without the data sets)')),
    (('--view-shift',), dict(default=0.1, type=float, metavar='FRAC', help='--mt-view geom: the shift is drawn from U(-FRAC, FRAC) times '
                            'the image side, per axis (0 .. 1; the default is a placeholder: its effect on convergence has not been '
                            'measured, and cannot be without the data sets)')),
    (('--view-margin',), dict(default=2.0, type=float, metavar='PX', help="--mt-view geom: a map takes part only when the teacher's "
                             'arg-max lies at least PX heat-map pixels inside its frame (0 <= PX < half the heat-map side; the default '
                             'is a placeholder: its effect on convergence has not been measured, and cannot be without the data sets)')),
    (('--fda',), dict(default='off', choices=['off', 'on'], help="Fourier-domain stylisation of the source batch (Fourier Domain "
                     "Adaptation, Yang and Soatto 2020; not in the reference): step A's forward takes every source image with the "
                     "amplitude of its (2b+1)^2 lowest frequencies replaced by that of the target image of the same index, the "
                     "phase -- and with it the geometry and the labels -- kept; two kernel launches at the head of step A, no "
                     "FFT, no extra pass through the network, no state.  Steps B, C and M and the pre-training step see the "
                     "images as the loaders deliver them.  Its effect on convergence has not been measured, and cannot be "
                     "without the data sets; 'off': nothing is launched")),
    (('--fda-beta',), dict(default=0.01, type=float, metavar='FLOAT', help='half-width of the swapped band as a fraction of the image '
                          'side: b = floor(--image-size * FLOAT) (positive; with --fda on, b <= 32 and 2b+1 <= --image-size; 0.01 is '
                          "the paper's smallest band and a placeholder: its effect on convergence has not been measured, and cannot "
                          'be without the data sets)')),
    (('--coord-loss',), dict(default='off', choices=['off', 'source', 'both'], help="coordinate loss on the differentiable soft-arg-max "
                            "(integral regression, Sun et al. 2018; not in the reference), one kernel launch per term: 'source' = step A "
                            "adds w * smooth-L1 between the soft-arg-max of softmax(beta * y_s) and the un-quantised annotation "
                            "(meta['keypoint2d'] in heat-map pixels), trained beside the heat-map losses through update A; 'both' = step "
                            "C also adds wt * the same loss between the target prediction and the EMA teacher's soft-arg-max on its "
                            "view of the target batch (needs --ema-update const|warmup; one teacher forward per iteration whatever "
                            "else uses it); 'off': nothing is launched.  The pre-training step keeps the KL alone")),
    (('--coord-weight',), dict(default=1.0, type=float, metavar='FLOAT', help='weight w of the source coordinate loss (constant, positive; '
                              'the default is a placeholder: its effect on convergence has not been measured, and cannot be without '
                              'the data sets)')),
    (('--coord-target-weight',), dict(default=1.0, type=float, metavar='FLOAT', help='weight wt of the target coordinate loss of '
                                     "--coord-loss both (constant, positive; the default is a placeholder: its effect on convergence "
                                     'has not been measured, and cannot be without the data sets)')),
    (('--coord-beta',), dict(default=1.0, type=float, metavar='FLOAT', help='inverse temperature of the softmax under the soft-arg-max '
                            '(positive; 1 = the distribution the KL loss trains the main head towards)')),
    (('--coord-delta',), dict(default=1.0, type=float, metavar='FLOAT', help='threshold of the smooth-L1 in heat-map pixels (0: plain L1)')),
    (('--bone-loss',), dict(default='off', choices=['off', 'on'], help="bone-ratio skeleton prior on the target batch (in the family "
                           "of the bone-length-ratio constraint of Zhou et al. 2017; not in the reference): step A blends the bone-length "
                           "ratios of the un-quantised source annotations (meta['keypoint2d']) into running statistics, step C adds w * "
                           "the squared excess beyond --bone-margin standard deviations of the same ratios of the target prediction's "
                           "soft-arg-max; no teacher and no further forward; the statistics travel in the epoch checkpoint (bone_state); "
                           "'off': nothing is launched")),
    (('--bone-weight',), dict(default=1.0, type=float, metavar='FLOAT', help='weight w of the bone-ratio prior (constant, positive; the '
                             'default is a placeholder: its effect on convergence has not been measured, and cannot be without the '
                             'data sets)')),
    (('--bone-margin',), dict(default=1.0, type=float, metavar='FLOAT', help='dead zone of the prior in standard deviations of the source '
                             'ratio (finite, not negative; a placeholder, as the weight)')),
    (('--bone-momentum',), dict(default=0.01, type=float, metavar='FLOAT', help='weight of a source batch in the running mean and variance '
                               'of the ratios, in [0, 1] (the first batch is taken whole; a placeholder, as the weight)')),
    (('--bone-beta',), dict(default=1.0, type=float, metavar='FLOAT', help='inverse temperature of the softmax under the soft-arg-max '
                           '(positive; a placeholder, as the weight)')),
    (('--bone-eps',), dict(default=1e-4, type=float, metavar='FLOAT', help='added to the running variance under the square root (positive; '
                          'a placeholder, as the weight)')),
    (('--occlude',), dict(default='off', choices=['off', 'keypoint'], help="adaptive key-point occlusion of the student's target input "
                         "(Kim et al. 2022; not in the reference): the EMA teacher's forward moves to the head of step B; with "
                         "probability --occlude-p per sample, square patches around up to --occlude-n key points the teacher is sure "
                         "of (peak of softmax(--conf-beta * y) >= --teacher-conf; valid under --mt-view geom; weight > 0) are set to the "
                         "data-set mean in the copy of the target batch the student's forwards read -- the teacher, step M's blend and "
                         "--fda keep the loader's images, and the training 'Acc (t)' meter then describes the occluded input.  The boxes "
                         "come from an RNG state of their own, seeded from --seed and the rank, kept in the epoch checkpoint "
                         "(occlude_state); needs --ema-update const|warmup; 'off': nothing is launched, nothing is drawn")),
    (('--occlude-p',), dict(default=0.5, type=float, metavar='FLOAT', help='--occlude keypoint: probability that a sample is occluded at all '
                           '(0 .. 1; the default is a placeholder: its effect on convergence has not been measured, and cannot be '
                           'without the data sets)')),
    (('--occlude-n',), dict(default=1, type=int, metavar='N', help='--occlude keypoint: at most N patches per occluded sample, around '
                           'distinct key points (1 .. 8; a placeholder, as the probability)')),
    (('--occlude-size',), dict(default=[0.08, 0.16], type=float, nargs=2, metavar=('LO', 'HI'), help='--occlude keypoint: the side of a patch '
                              'is drawn uniformly from LO .. HI times --image-size, in whole pixels (0 < LO <= HI <= 1; a placeholder, as '
                              'the probability)')),
    (('--teacher-conf',), dict(default=0.0, type=float, metavar='TAU', help="a teacher map counts for --mt-loss, --coord-loss both and "
                              "--mixup-labels teacher only when the peak of softmax(--conf-beta * y) reaches TAU (the flags multiply in "
                              "where the flags of --mt-view geom do); also the candidate threshold of --occlude keypoint.  A perfect "
                              "sigma = 2 label has a peak of 1 / (8 pi) = 0.0398.  0: no gate, nothing is launched (the default; any "
                              "other value is a placeholder: its effect on convergence has not been measured, and cannot be without "
                              "the data sets)")),
    (('--conf-beta',), dict(default=1.0, type=float, metavar='FLOAT', help='inverse temperature of the softmax whose peak is the '
                           "teacher's confidence (positive; 1 = the distribution the KL loss trains the main head towards; a "
                           'placeholder, as the threshold)')),
    (('--clip-grad-norm',), dict(default=0.0, type=_clip_norm, metavar='FLOAT', help="global gradient-norm clipping with a non-finite "
                                "step guard: each of the updates A, B, C (M with --mixup on; and the pre-training step) clips over everything it steps, as "
                                "clip_grad_norm_(those parameters, FLOAT) before the optimizers would, in two launches per update and "
                                "inside the SGD kernels; an update whose norm is inf or NaN is skipped and counted ('skipped steps:'); "
                                "'inf' measures and guards without scaling; 0: off, nothing is launched")),
    (('--optimizer',), dict(default='sgd', choices=['sgd', 'adam', 'adamw'], help="every optimizer of the run, the pre-training one "
                           "included: 'sgd' = SGD with Nesterov momentum (the reference); 'adam' = Adam with --wd as L2 weight decay; "
                           "'adamw' = Adam with --wd as decoupled weight decay -- both in two launches per update over the flat "
                           "buffers (mi355.optim.FusedAdam), with the same schedules, --clip-grad-norm, --ema-update and --*-loss "
                           "terms; --momentum is ignored by both.  The learning rate reached through --lr is a placeholder under "
                           "adam / adamw (recipes use about 1e-3): its effect on convergence has not been measured, and cannot be "
                           "without the data sets.  --resume takes a checkpoint of the same kind only")),
    (('--adam-betas',), dict(default=(0.9, 0.999), type=float, nargs=2, metavar=('B1', 'B2'), help='Adam coefficients of the running '
                            'averages of the gradient and of its square (--optimizer adam | adamw; each in [0, 1))')),
    (('--adam-eps',), dict(default=1e-8, type=float, metavar='FLOAT', help="term added to Adam's denominator (--optimizer adam | adamw)")),
    (('--no-graph',), dict(action='store_true', help='launch kernels eagerly instead of replaying HIP graphs')),
    (('--metrics',), dict(default='pck', choices=['pck', 'full'], help="'full': validation also decodes key points in image pixels "
                         "and reports the mean end-point error, the PCK curve's AUC and per-group EPEs (on the device, one read at "
                         "the end); 'pck': the reference's heat-map PCK alone")),
    (('--decode',), dict(default='argmax', choices=['argmax', 'upsample', 'quarter', 'taylor'], help="key points of --metrics full: "
                        "'argmax' = heat-map arg-max times image / heat-map size; 'upsample' = arg-max of the heat-maps up-sampled "
                        "bilinearly to the image size (compute_uv_from_heatmaps2), in one kernel; 'quarter' = the arg-max moved a "
                        "quarter heat-map pixel towards its higher neighbour; 'taylor' = the second-order (DARK) step on the log of "
                        "the smoothed heat-map, exact for Gaussian labels")),
    (('--decode-sigma',), dict(default=None, type=float, metavar='FLOAT', help="Gaussian of the smoothing in front of --decode taylor "
                              "(default: the sigma of the data set's labels)")),
    (('--flip-test',), dict(action='store_true', help='validation / test: average the heat-maps of every image with those of its mirror '
                           'image (one forward of twice the batch); the loss, the heat-map PCK and the --metrics full decode use the average')),
    (('--flip-shift',), dict(default=1, type=int, choices=[0, 1], help="columns the mirrored heat-maps move to the right before they "
                            "are averaged (1: Simple Baselines' SHIFT_HEATMAP, the alignment of a 4x down-sampled map; 0: plain mirror)")),
    (('--auc-max-px',), dict(default=30.0, type=float, metavar='FLOAT', help='upper end of the PCK thresholds of --metrics full (0 .. this, 31 steps)')),
    (('--device-augment',), dict(action='store_true', help='run the training augmentation chain (rotate, resized crop, colour '
                                  'jitter, blur, normalisation), the validation resize + normalisation and the heat-map labels '
                                  'of both on the GPU, bit-exact with the CPU chains; the loader workers (validation included) '
                                  'only decode, crop (RHD / STB) and draw the parameters')),
]


class _Parser(argparse.ArgumentParser):
    """Checks between flags that argparse cannot express."""

    def parse_args(self, *a, **kw):
        args = super().parse_args(*a, **kw)
        if getattr(args, 'synthetic_hands', False):
            if getattr(args, 'synthetic', False):
                self.error('--synthetic and --synthetic-hands exclude each other: noise batches or rendered hands, not both')
            if getattr(args, 'device_augment', False):
                self.error('--device-augment with --synthetic-hands: the rendered records already are the device path '
                           '(images and labels are made on the GPU); drop --device-augment')
            if min(args.render_train_size, args.render_val_size) < 1:
                self.error('--render-train-size and --render-val-size must be at least 1')
            if args.image_size % 16 != 0 or not 16 <= args.image_size <= 512:
                self.error('--synthetic-hands renders sides that are multiples of 16 from 16 to 512, got --image-size %d' % args.image_size)
        if not 0.0 <= getattr(args, 'render_gap', 1.0) <= 1.0:
            self.error('--render-gap must lie in 0 .. 1, got %r' % (args.render_gap,))
        if getattr(args, 'mt_loss', 'off') == 'on' and getattr(args, 'ema_update', 'off') == 'off':
            self.error('--mt-loss on needs a moving teacher: add --ema-update const (or warmup)')
        if getattr(args, 'mixup', 'off') == 'on' and getattr(args, 'mixup_labels', 'student') == 'teacher' and \
                getattr(args, 'ema_update', 'off') == 'off':
            self.error('--mixup-labels teacher needs a moving teacher: add --ema-update const (or warmup)')
        if getattr(args, 'coord_loss', 'off') == 'both' and getattr(args, 'ema_update', 'off') == 'off':
            self.error('--coord-loss both needs a moving teacher: add --ema-update const (or warmup)')
        if getattr(args, 'mt_view', 'same') == 'geom':
            if not (getattr(args, 'mt_loss', 'off') == 'on' or getattr(args, 'coord_loss', 'off') == 'both' or
                    (getattr(args, 'mixup', 'off') == 'on' and getattr(args, 'mixup_labels', 'student') == 'teacher')):
                self.error("--mt-view geom changes what the teacher's forward sees, and nothing reads that forward: add --mt-loss on, "
                           "--coord-loss both or --mixup on --mixup-labels teacher")
            if getattr(args, 'ema_update', 'off') == 'off':
                self.error('--mt-view geom needs a moving teacher: add --ema-update const (or warmup)')
        consumer = getattr(args, 'mt_loss', 'off') == 'on' or getattr(args, 'coord_loss', 'off') == 'both' or \
            (getattr(args, 'mixup', 'off') == 'on' and getattr(args, 'mixup_labels', 'student') == 'teacher')
        if getattr(args, 'occlude', 'off') == 'keypoint' and getattr(args, 'ema_update', 'off') == 'off':
            self.error('--occlude keypoint needs a moving teacher: add --ema-update const (or warmup)')
        if getattr(args, 'teacher_conf', 0.0) > 0 and not (consumer or getattr(args, 'occlude', 'off') == 'keypoint'):
            self.error("--teacher-conf gates the teacher's maps, and nothing reads them: add --mt-loss on, --coord-loss both, "
                       "--mixup on --mixup-labels teacher or --occlude keypoint")
        try:                                             # (the checks the term classes make, under the flags' names)
            if getattr(args, 'teacher_conf', None) is not None:
                if not 0.0 <= args.teacher_conf < float('inf'):
                    raise ValueError('--teacher-conf must be finite and not negative, got %r' % (args.teacher_conf,))
                if not 0.0 < args.conf_beta < float('inf'):
                    raise ValueError('--conf-beta must be finite and positive, got %r' % (args.conf_beta,))
            if getattr(args, 'occlude', 'off') == 'keypoint':
                lo, hi = args.occlude_size
                if not 0.0 <= args.occlude_p <= 1.0:
                    raise ValueError('--occlude-p must lie in 0 .. 1, got %r' % (args.occlude_p,))
                if not 1 <= args.occlude_n <= 8:
                    raise ValueError('--occlude-n must lie in 1 .. 8, got %r' % (args.occlude_n,))
                if not (0.0 < lo <= hi <= 1.0):
                    raise ValueError('--occlude-size needs 0 < LO <= HI <= 1 (fractions of --image-size), got %r %r' % (lo, hi))
                if int(args.image_size) % int(getattr(args, 'heatmap_size', 64)) != 0:
                    raise ValueError('--occlude keypoint needs --image-size to be a multiple of --heatmap-size, got %r and %r'
                                     % (args.image_size, getattr(args, 'heatmap_size', 64)))
            if getattr(args, 'mt_view', 'same') == 'geom':
                lo, hi = args.view_scale
                if not 0.0 <= args.view_rot <= 180.0:
                    raise ValueError('--view-rot must lie in 0 .. 180 degrees, got %r' % (args.view_rot,))
                if not (0.0 < lo <= hi < float('inf')):
                    raise ValueError('--view-scale needs finite 0 < LO <= HI, got %r %r' % (lo, hi))
                if not 0.0 <= args.view_shift <= 1.0:
                    raise ValueError('--view-shift is a fraction of the image side in 0 .. 1, got %r' % (args.view_shift,))
                if not 0.0 <= args.view_margin < 0.5 * float(getattr(args, 'heatmap_size', 64)):
                    raise ValueError('--view-margin must lie in 0 .. half of --heatmap-size, got %r' % (args.view_margin,))
            if getattr(args, 'mixup', 'off') == 'on':
                check_positive('--mixup-beta', args.mixup_beta)
                check_positive('--mixup-weight', args.mixup_weight)
            if getattr(args, 'fda_beta', None) is not None:
                check_positive('--fda-beta', args.fda_beta)
                if getattr(args, 'fda', 'off') == 'on':
                    side = int(args.image_size)
                    b = fda_band(side, side, args.fda_beta)
                    if b > FDA_MAX_B:
                        raise ValueError('--fda-beta: beta = %g gives b = %d at --image-size %d, above the limit of %d' % (args.fda_beta, b, side, FDA_MAX_B))
                    if 2 * b + 1 > side:
                        raise ValueError('--fda-beta: beta = %g gives b = %d: the window 2b+1 = %d is wider than the limit of --image-size %d'
                                         % (args.fda_beta, b, 2 * b + 1, side))
            if getattr(args, 'coord_loss', 'off') != 'off':
                check_positive('--coord-weight', args.coord_weight)
                check_positive('--coord-target-weight', args.coord_target_weight)
                check_positive('--coord-beta', args.coord_beta)
                if not 0.0 <= args.coord_delta < float('inf'):
                    raise ValueError('--coord-delta must be finite and not negative, got %r' % (args.coord_delta,))
            if getattr(args, 'bone_loss', 'off') == 'on':
                check_positive('--bone-weight', args.bone_weight)
                check_positive('--bone-beta', args.bone_beta)
                check_positive('--bone-eps', args.bone_eps)
                if not 0.0 <= args.bone_margin < float('inf'):
                    raise ValueError('--bone-margin must be finite and not negative, got %r' % (args.bone_margin,))
                if not 0.0 <= args.bone_momentum <= 1.0:
                    raise ValueError('--bone-momentum must be in [0, 1], got %r' % (args.bone_momentum,))
            if getattr(args, 'mmd_loss', 'off') == 'on':
                check_positive('--mmd-weight', args.mmd_weight)
                check_whole('--mmd-kernels', args.mmd_kernels, 8)
                check_positive('--mmd-mul', args.mmd_mul)
                if args.batch_size > 128:
                    self.error('--mmd-loss on takes at most 128 images per domain and GPU (the kernels hold n = 2 B <= 256 rows), got -b %d' % args.batch_size)
            if getattr(args, 'jfa_loss', 'off') == 'on':
                check_positive('--jfa-weight', args.jfa_weight)
                check_whole('--jfa-radius', args.jfa_radius, 16)
            if getattr(args, 'proto_loss', 'off') != 'off':
                check_positive('--proto-weight', args.proto_weight)
                check_whole('--proto-radius', args.proto_radius, 16)
                check_blend_weight('--proto-m', args.proto_m)
            if getattr(args, 'optimizer', 'sgd') != 'sgd':
                for i, b in enumerate(args.adam_betas):
                    if not 0.0 <= b < 1.0:
                        raise ValueError('--adam-betas: Invalid beta parameter at index %d: %r' % (i, b))
                if not 0.0 <= args.adam_eps:
                    raise ValueError('--adam-eps: Invalid epsilon value: %r' % (args.adam_eps,))
        except ValueError as e:
            self.error(str(e))
        if getattr(args, 'dump_preds', None):
            args.metrics = 'full'                        # (test.py: predictions are what --metrics full decodes)
        if getattr(args, 'decode', 'argmax') != 'argmax' and getattr(args, 'metrics', 'pck') != 'full':
            self.error('--decode %s decodes the key points of --metrics full: add --metrics full' % args.decode)
        return args


def build_parser(description='Domain-adaptive hand-pose training on MI355X'):
    archs = sorted(n for n in models.__dict__ if n.islower() and not n.startswith('__') and callable(models.__dict__[n]))
    parser = _Parser(description=description)
    parser.add_argument('-a', '--arch', metavar='ARCH', default='resnet101', choices=archs, help=' | '.join(archs))
    for flags, kw in _OPTIONS:
        parser.add_argument(*flags, **kw)
    return parser


if __name__ == '__main__':
    main(build_parser().parse_args())
