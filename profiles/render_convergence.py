"""What a short run learns from the rendered hand data set (DESIGN.md section 7 "Rendered hands"): five recorded runs of train1.py /
test.py, one row each, evaluated with --metrics full on the 'cg' and on the 'photo' validation set of --synthetic-hands:

  1 untrained          the model as built, nothing loaded
  2 noise              a run on --synthetic noise (--noise-pre-iters of pre-training, then row 4's adversarial length): the chance
                       yardstick -- its loader is CPU-bound, so its pre-training is kept short; more noise teaches nothing more
  3 source_only        pre-training on the rendered 'cg' set alone
  4 adversarial        row 3's weights, then the reference's adversarial loop on 'cg' -> 'photo'
  5 adversarial_gap0   as 4 at --render-gap 0 (evaluated on a 'photo' set at gap 0: the same distribution as 'cg')

ResNet-18 from random weights, fixed seed, sized to finish in minutes; iteration counts and wall times are part of the result.  No
adaptation switch is on in any row.  --lr defaults to 0.1, not train1.py's 0.01: the pre-training gives the backbone a tenth of
--lr (it fine-tunes ImageNet weights in the reference), and a backbone that starts from random weights does not leave the
constant-map plateau in a few thousand iterations at 0.001.  The pre-training curve of row 3 (loss, training and validation
accuracy per epoch) is part of the result.  Prints one line per row and, last, one JSON line with all.

    python profiles/render_convergence.py [--size 128] [-b 32] [--lr 0.1] [--pre-iters 2000] [--noise-pre-iters 300] [--iters 200] [--json PATH]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd')


def run(script, argv, limit):
    t0 = time.time()
    r = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.join(PKG, script)] + argv, env=dict(os.environ, PYTHONPATH=PKG),
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit('%s %s failed (%d):\n%s' % (script, ' '.join(argv), r.returncode, (r.stdout + r.stderr)[-3000:]))
    return r.stdout, time.time() - t0


def figures(out):
    """PCK (the 'all' accuracy) and EPE of the last source / target evaluation in a train1.py / test.py log."""
    pck = re.findall(r'^Source: ([0-9.]+) Target: ([0-9.]+)', out, flags=re.M)[-1]
    epe = re.findall(r'^EPE: ([^ ]+) px', out, flags=re.M)
    src, tgt = epe[-2], epe[-1]
    return {'pck_cg': float(pck[0]), 'pck_photo': float(pck[1]), 'epe_cg_px': float(src), 'epe_photo_px': float(tgt)}


def pretraining_curve(out):
    """Per pre-training epoch: the last printed training loss and heat-map accuracy (running means) and the 'cg' validation accuracy."""
    head = out.split('Start regression domain adaptation.')[0]
    curve = []
    for e, acc in enumerate(re.findall(r'^Source: ([0-9.eE+-]+) best: ', head, flags=re.M)):
        lines = re.findall(r'^Epoch: \[%d\]\[\s*\d+/\d+\].*?Loss \(s\) \S+ \((\S+)\)\s+Acc \(s\) \S+ \((\S+)\)' % e, head, flags=re.M)
        loss, tacc = lines[-1] if lines else (None, None)
        curve.append({'epoch': e, 'train_loss': float(loss) if loss else None, 'train_acc': float(tacc) if tacc else None, 'val_acc_cg': float(acc)})
    return curve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='resnet18')
    ap.add_argument('--size', type=int, default=128, help='image side; the heat-maps are a quarter of it')
    ap.add_argument('-b', type=int, default=32)
    ap.add_argument('--pre-iters', type=int, default=2000, help='pre-training iterations (rows 3 - 5), in epochs of 100')
    ap.add_argument('--noise-pre-iters', type=int, default=300, help='pre-training iterations of row 2, in epochs of 100')
    ap.add_argument('--lr', type=float, default=0.1, help='--lr of every run (module docstring)')
    ap.add_argument('--iters', type=int, default=200, help='adversarial iterations (rows 2, 4, 5), in epochs of 100')
    ap.add_argument('--val', type=int, default=256)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('-j', type=int, default=2, help='loader workers per data set')
    ap.add_argument('--limit', type=int, default=420, help='time limit of one child run, seconds')
    ap.add_argument('--json', default=None, help='also write the result line to this file')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: nothing is measured without one')
    common = ['data/none', '-t', 'Hand3DStudio', '-a', a.arch, '-b', str(a.b), '-i', '100', '-p', '50', '-j', str(a.j), '--seed', str(a.seed), '--lr', str(a.lr),
              '--image-size', str(a.size), '--heatmap-size', str(a.size // 4), '--metrics', 'full', '--render-val-size', str(a.val)]
    hands = ['--synthetic-hands']
    pre_epochs, epochs, noise_epochs = max(a.pre_iters // 100, 1), max(a.iters // 100, 1), max(a.noise_pre_iters // 100, 1)
    res = {'arch': a.arch, 'image': a.size, 'heatmap': a.size // 4, 'batch': a.b, 'seed': a.seed, 'lr': a.lr, 'noise_pretrain_iterations': noise_epochs * 100, 'val_items_per_domain': a.val,
           'pretrain_iterations': pre_epochs * 100, 'adversarial_iterations': epochs * 100, 'auc_max_px': 30.0, 'rows': {}}
    with tempfile.TemporaryDirectory() as tmp:
        empty = os.path.join(tmp, 'empty.pth')
        torch.save({'model': {}}, empty)

        def row(name, out, secs, note):
            res['rows'][name] = dict(figures(out), wall_s=round(secs, 1), note=note)
            print('%-18s %s' % (name, json.dumps(res['rows'][name])), flush=True)

        out, s = run('train1.py', common + hands + ['--phase', 'test', '--pretrain', empty, '--log', os.path.join(tmp, 'r1')], a.limit)
        row('untrained', out, s, 'nothing loaded, nothing trained')
        log2 = os.path.join(tmp, 'r2')
        _, s2 = run('train1.py', common + ['--synthetic', '--pretrain_epochs', str(noise_epochs), '--epochs', str(epochs), '--pretrain',
                                           os.path.join(tmp, 'none2.pth'), '--log', log2], a.limit)
        out, s = run('test.py', common + hands + ['--checkpoint', os.path.join(log2, 'checkpoints', '%d.pth' % (epochs - 1)), '--log', os.path.join(tmp, 'r2t')], a.limit)
        row('noise', out, s2 + s, 'trained on --synthetic noise (%d + %d iterations), evaluated on the rendered sets' % (noise_epochs * 100, epochs * 100))
        log3 = os.path.join(tmp, 'r3')
        out, s = run('train1.py', common + hands + ['--pretrain_epochs', str(pre_epochs), '--phase', 'test', '--pretrain', os.path.join(tmp, 'none3.pth'),
                                                    '--log', log3], a.limit)
        row('source_only', out, s, "pre-training on 'cg' alone, %d iterations; the best epoch by 'cg' validation accuracy is kept" % (pre_epochs * 100))
        res['rows']['source_only']['pretraining_curve'] = pretraining_curve(out)
        pre = os.path.join(log3, 'checkpoints', 'pretrain.pth')
        for name, gap in (('adversarial', '1.0'), ('adversarial_gap0', '0.0')):
            out, s = run('train1.py', common + hands + ['--render-gap', gap, '--pretrain', pre, '--epochs', str(epochs), '--log', os.path.join(tmp, name)], a.limit)
            row(name, out, s, "row source_only's weights, then %d iterations of the adversarial loop at --render-gap %s" % (epochs * 100, gap))
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
