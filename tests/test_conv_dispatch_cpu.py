"""The choice of a conv kernel build, without a GPU: tests/conv_dispatch_probe.cpp drives csrc/conv_plan.h (describe, choose,
tile grid / epilogue admission, weight-gradient plan) and prints what the launch log would show in brackets; this module holds
that against the expected-build tables of conv_exact_ref.py -- the tables test_gpu_conv_exact.py asserts on the real launches --
for every case, under the case's group environment.  A threshold edit that moves a case to another build fails here first.

The probe is a stand-alone host program built with AddressSanitizer + UndefinedBehaviorSanitizer; a report fails the test."""
import importlib.util
import os
import re
import subprocess

import pytest
import torch

import conv_exact_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd')
DT = {'bf16': torch.bfloat16, 'f32': torch.float32}


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    spec = importlib.util.spec_from_file_location('mi355_build', os.path.join(PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe = str(tmp_path_factory.mktemp('probe') / 'conv_dispatch_probe')
    cmd = [os.path.join(mod.LLVM_BIN, 'clang++'), '-std=c++17', '-Wall', '-Werror', '-O1', '-g', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', os.path.join(ROOT, 'tests', 'conv_dispatch_probe.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _expand(expect):
    """'build *4' -> four launches of it (one per phase, MI355_PHASES=0)."""
    if ' *' in expect:
        return [expect.split(' *')[0]] * int(expect.split(' *')[1])
    return [expect]


def _bare(build):
    return re.sub(r' epi\d$', '', build)


def _epi(builds):
    """The epilogue index the launches of one call carry: one for all of them."""
    epis = set(int(b[-1]) if re.search(r' epi\d$', b) else 0 for b in builds)
    assert len(epis) == 1, builds
    return epis.pop()


def _lines(group):
    """[(what, probe line, check)] for every case of `group`; check(builds) asserts on the builds the probe printed."""
    out = []

    def exact(expect):
        return lambda got: got == expect

    def with_epi(expect, epi, always):
        # the bare builds as expected; the epilogue fused (always, or where the phases allow it) or refused, never half done
        return lambda got: [_bare(b) for b in got] == expect and (_epi(got) == epi if always else _epi(got) in (0, epi))

    for name, (g, N, Ci, H, W, Co, k, s, p, out_hw, dgrad) in R.CASES.items():
        if g != group:
            continue
        Ho, Wo = out_hw if out_hw is not None else R.out_size(H, W, k, k, s, p)
        for i, dt in enumerate(('bf16', 'f32')):
            e_fwd, e_dgrad, e_acc, e_bnb, e_wgrad = R.EXPECT[name][i]
            shape = '%s %d %d %d %d %d %d %d %d %d %d' % (dt, N, H, W, Ci, Co, k, s, p, Ho, Wo)
            tag = '%s/%s ' % (name, dt)
            out += [(tag + 'fwd', 'fwd ' + shape, exact([e_fwd])),
                    (tag + 'fwd+res', 'fwd ' + shape + ' res=1', exact([e_fwd])),
                    (tag + 'fwd+stats', 'fwd ' + shape + ' stats=1', exact([e_fwd + ' epi1'])),
                    (tag + 'wgrad', 'wgrad ' + shape, exact([e_wgrad]))]
            if dgrad:
                out += [(tag + 'dgrad', 'dgrad ' + shape, exact(_expand(e_dgrad))),
                        (tag + 'dgrad+acc', 'dgrad ' + shape + ' acc=1', exact(_expand(e_acc))),
                        (tag + 'dgrad+macc', 'dgrad ' + shape + ' acc=2', exact(_expand(e_acc))),
                        (tag + 'dgrad+stats', 'dgrad ' + shape + ' stats=1', with_epi(_expand(e_dgrad), 1, s == 1)),
                        (tag + 'dgrad+bnb', 'dgrad ' + shape + ' bnb=1', with_epi(_expand(e_bnb), 2, s == 1))]
    for name, (g, N, Ci, H, W, Co, k, s, p) in R.CAT_CASES.items():
        if g != group:
            continue
        Ho, Wo = R.out_size(H, W, k, k, s, p)
        for i, dt in enumerate(('bf16', 'f32')):
            for c2 in R.CAT_C2[DT[dt]]:
                line = 'cat %s %d %d %d %d %d %d %d %d %d %d c2=%d' % (dt, N, H, W, Ci, Co, k, s, p, Ho, Wo, c2)
                tag = '%s/%s c2=%d ' % (name, dt, c2)
                out += [(tag + 'cat', line, exact([R.CAT_EXPECT[name][i]])),
                        (tag + 'cat+stats', line + ' stats=1', exact([R.CAT_EXPECT[name][i] + ' epi1']))]
    for name, (g, N, Ci, H, W, Co, k, s, p) in R.FP8_CASES.items():
        if g != group:
            continue
        Ho, Wo = R.out_size(H, W, k, k, s, p)
        shape = ' bf16 %d %d %d %d %d %d %d %d %d %d' % (N, H, W, Ci, Co, k, s, p, Ho, Wo)
        e_plain, e_kw3 = R.FP8_EXPECT[name]
        e_fwd, e_dgrad = e_plain if isinstance(e_plain, tuple) else (e_plain, e_plain)
        for mode, ef, ed in ((0, e_fwd, e_dgrad), (1, e_kw3, e_kw3)):
            if ef is None:
                continue
            tag, kw = '%s kw3=%d ' % (name, mode), ' kw3min=%d' % mode
            out += [(tag + 'fwd8+stats', 'fp8' + shape + kw + ' stats=1', exact(['f8 ' + ef + ' epi1'])),
                    (tag + 'fwd8', 'fp8' + shape + kw, exact(['f8 ' + ef])),
                    (tag + 'dgrad8', 'fp8:dgrad' + shape + kw, exact(['f8 ' + ed + ' bf8'])),
                    (tag + 'dgrad8+stats', 'fp8:dgrad' + shape + kw + ' stats=1', with_epi(['f8 ' + ed + ' bf8'], 1, s == 1)),
                    (tag + 'dgrad8+acc', 'fp8:dgrad' + shape + kw + ' acc=1', exact(['f8 ' + ed + ' bf8']))]
        out += [(name + ' fwdmx+stats', 'mx' + shape + ' stats=1', exact(['mx ' + e_fwd + ' epi1'])),
                (name + ' fwdmx', 'mx' + shape, exact(['mx ' + e_fwd])),
                (name + ' dgradmx', 'mx:dgrad' + shape, exact(['mx ' + e_dgrad])),
                (name + ' dgradmx+stats', 'mx:dgrad' + shape + ' stats=1', with_epi(['mx ' + e_dgrad], 1, s == 1)),
                (name + ' dgradmx+acc', 'mx:dgrad' + shape + ' acc=1', exact(['mx ' + e_dgrad]))]
    for (N, H, W, Co, pg), expect in zip(R.ROUNDING_CASES.get(group, []), R.ROUNDING_EXPECT.get(group, [])):
        line = 'fwd bf16 %d %d %d 64 %d 1 1 0 %d %d' % (N, H, W, Co, H, W) + ('' if pg is None else ' pgemm=%d' % pg)
        out.append(('rounding %s' % ((N, H, W, Co, pg),), line, exact([expect])))
    if group == 'default':
        for name, (N, Ci, H, W, Co, dgrad) in R.PGEMM_CASES.items():
            shape = ' bf16 %d %d %d %d %d 1 1 0 %d %d' % (N, H, W, Ci, Co, H, W)
            e_fwd, e_dgrad = R.PGEMM_EXPECT[name]
            out += [(name + ' fwd', 'pgemm' + shape, exact([e_fwd[0]])),
                    (name + ' fwd+res', 'pgemm' + shape + ' res=1', exact([e_fwd[1]])),
                    (name + ' fwd+stats', 'pgemm' + shape + ' stats=1', exact([e_fwd[0] + ' epi1']))]
            if dgrad:
                out += [(name + ' dgrad', 'pgemm:dgrad' + shape, exact([e_dgrad[0]])),
                        (name + ' dgrad+acc', 'pgemm:dgrad' + shape + ' acc=1', exact([e_dgrad[1]])),
                        (name + ' dgrad+macc', 'pgemm:dgrad' + shape + ' acc=2', exact([e_dgrad[1]]))]
    return out


@pytest.mark.parametrize('group', ['default'] + sorted(R.GROUPS))
def test_chooser_names_the_expected_build(probe, group):
    cases = _lines(group)
    assert cases, group
    env = {k: v for k, v in os.environ.items() if not k.startswith('MI355_')}
    env.update(R.GROUPS.get(group, {}), ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([probe], input=''.join(c[1] + '\n' for c in cases), capture_output=True, text=True, env=env, timeout=120)
    report = (r.stdout[-2000:] + r.stderr[-4000:])
    assert 'Sanitizer' not in report and 'runtime error:' not in report and r.returncode == 0, report
    got = {}
    for row in r.stdout.splitlines():
        n, text = row.split('\t')
        got.setdefault(int(n), []).append(text)
    wrong = ['%s: `%s` -> %r' % (what, line, got.get(i + 1, [])) for i, (what, line, check) in enumerate(cases) if not check(got.get(i + 1, []))]
    assert not wrong, '%d of %d choices differ from the tables of conv_exact_ref.py:\n%s' % (len(wrong), len(cases), '\n'.join(wrong))


def test_every_case_belongs_to_a_group_that_runs():
    groups = set(['default'] + list(R.GROUPS))
    for table in (R.CASES, R.CAT_CASES, R.FP8_CASES):
        assert set(v[0] for v in table.values()) <= groups
    assert set(R.CASES) == set(R.EXPECT) and set(R.CAT_CASES) == set(R.CAT_EXPECT) and set(R.FP8_CASES) == set(R.FP8_EXPECT)
    assert set(R.PGEMM_CASES) == set(R.PGEMM_EXPECT) and set(R.ROUNDING_CASES) == set(R.ROUNDING_EXPECT)


# ---------------------------------------------------------------------------------------------- what the guard buffers need
def _probe(probe, lines, group='default'):
    """{line number: [texts]} of the probe for `lines` under the environment of `group`."""
    env = {k: v for k, v in os.environ.items() if not k.startswith('MI355_')}
    env.update(R.GROUPS.get(group, {}), ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([probe], input=''.join(l + '\n' for l in lines), capture_output=True, text=True, env=env, timeout=120)
    report = (r.stdout[-2000:] + r.stderr[-4000:])
    assert 'Sanitizer' not in report and 'runtime error:' not in report and r.returncode == 0, report
    got = {}
    for row in r.stdout.splitlines():
        n, text = row.split('\t')
        got.setdefault(int(n), []).append(text)
    return got


# The cases of conv_exact_ref.py that give the poisoned guard buffers of test_gpu_conv_exact.py (tests/guarded.py) something to
# find, named so that a table edit which loses one fails here: (a) weight gradients whose last split is ragged, (b) one slab
# with accumulate (the slab path with a single slab), (c) a grouped launch with more than one slab-reduced item, (d) statistics
# epilogues that fill fewer slices than their buffer holds.
GUARD_COVERAGE = {
    'ragged':       [('small7', 'bf16'), ('t64x128', 'f32'), ('kg2_64', 'bf16'), ('wkw2_wo8', 'bf16')],
    'single_slab':  [('wkw_direct', 'bf16'), ('wkw2_direct', 'bf16'), ('wgen_direct', 'bf16')],
    'grouped':      [('wgrad_group', 'f32', 0), ('wgrad_kw_group', 'bf16', 1)],        # (form, format, index of the launch)
    'slices':       ['small7', 't64x128', 'kg2_128', 't256d', 'kw3_256x128'],
}


def test_the_cases_give_the_guard_buffers_something_to_find(probe):
    # (a), (b): plan_wgrad / wgrad_split of the single launches
    names = sorted(set(GUARD_COVERAGE['ragged'] + GUARD_COVERAGE['single_slab']))
    lines = []
    for name, dt in names:
        g, N, Ci, H, W, Co, k, s, p, out_hw, dgrad = R.CASES[name]
        assert g == 'default'
        Ho, Wo = out_hw if out_hw is not None else R.out_size(H, W, k, k, s, p)
        lines.append('wplan %s %d %d %d %d %d %d %d %d %d %d' % (dt, N, H, W, Ci, Co, k, s, p, Ho, Wo))
    got = _probe(probe, lines)
    plan = {}
    for i, key in enumerate(names):
        m = re.match(r'(\w+) S(\d+) rows(\d+) M(\d+) ws(\d+)$', got[i + 1][0])
        assert m, got[i + 1]
        plan[key] = (m.group(1),) + tuple(int(v) for v in m.groups()[1:])
        kernel, S, rows, M, ws = plan[key]
        assert '%s S%d' % (kernel, S) == R.EXPECT[key[0]][0 if key[1] == 'bf16' else 1][4]          # the launch the GPU test pins
        assert (S - 1) * rows < M <= S * rows                                                        # no empty split
    for key in GUARD_COVERAGE['ragged']:
        kernel, S, rows, M, ws = plan[key]
        assert S > 1 and M % rows != 0, (key, plan[key])          # the last split holds fewer rows than the others
    assert len(set(plan[key][0] for key in GUARD_COVERAGE['ragged'])) == 3          # ... on each of the three kernels
    for key in GUARD_COVERAGE['single_slab']:
        kernel, S, rows, M, ws = plan[key]
        assert S == 1 and ws > 0, (key, plan[key])          # with accumulate (every case runs it) the one slab goes through the workspace
    assert len(set(plan[key][0] for key in GUARD_COVERAGE['single_slab'])) == 3

    # (c): walk_wgrad_groups / group_plan of the grouped calls
    for form, dt, launch in GUARD_COVERAGE['grouped']:
        fmts, shapes = R.GROUPED_CASES[form]
        assert dt in fmts
        lines, dw = [], {}
        for i, (N, H, W, Ci, Co, k, s, p, acc, share) in enumerate(shapes):
            Ho, Wo = R.out_size(H, W, k, k, s, p)
            dw[i] = dw[share] if share is not None else i
            lines.append('gitem %s %d %d %d %d %d %d %d %d %d %d acc=%d dw=%d' % (dt, N, H, W, Ci, Co, k, s, p, Ho, Wo, int(acc), dw[i]))
        got = _probe(probe, lines + ['gplan'])[len(lines) + 1]
        head, items = got[launch].split(' | ')[0], got[launch].split(' | ')[1:]
        assert head.startswith('kind') and head[4] in '123', got
        slabbed = [it for it in items if it.endswith(' slab1')]
        assert len(slabbed) > 1, (form, got)          # two slab regions of one workspace side by side, one grouped reduction
        split = [it for it in slabbed if int(re.search(r' S(\d+) ', it).group(1)) > 1]
        print('\nGROUPED %s/%s launch %d: %s (%d slab-reduced, %d of them split)' % (form, dt, launch, got[launch], len(slabbed), len(split)))

    # (d): plan_tile_grid of the statistics epilogues
    lines = []
    for name in GUARD_COVERAGE['slices']:
        g, N, Ci, H, W, Co, k, s, p, out_hw, dgrad = R.CASES[name]
        Ho, Wo = out_hw if out_hw is not None else R.out_size(H, W, k, k, s, p)
        lines.append('fwd bf16 %d %d %d %d %d %d %d %d %d %d stats=1 slices=1' % (N, H, W, Ci, Co, k, s, p, Ho, Wo))
    got = _probe(probe, lines)
    for i, name in enumerate(GUARD_COVERAGE['slices']):
        m = re.search(r'^(.*) epi1 slices=(\d+)/(\d+)$', got[i + 1][0])
        assert m and m.group(1) == R.EXPECT[name][0][0], got[i + 1]
        assert 1 <= int(m.group(2)) < int(m.group(3)), got[i + 1]          # slices behind the last written one: they must stay untouched
