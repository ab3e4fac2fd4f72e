"""The rendered hand data set without a GPU: the kinematic model (utils/hand_model.py), the records and the two domains
(utils/rendered_dataset.py), the numpy restatement of the image definition (tests/render_ref.py) on ordinary and degenerate
records, and the command-line checks of --synthetic-hands."""
import warnings

import numpy as np
import pytest

import render_ref as R


def _ds(**kw):
    from utils.rendered_dataset import RenderedHand21
    return RenderedHand21(**dict(dict(length=4096, image_size=64, heatmap_size=16, seed=7), **kw))


def test_bone_lengths_are_rest_length_times_the_finger_factor_whatever_the_pose():
    from utils import hand_model as hm
    from uda.model.loss import HAND_BONES
    rest, finger = hm.rest_lengths(), hm.bone_finger()
    assert len(HAND_BONES) == 20 and rest.shape == (20,) and (rest > 0).all()
    for seed in range(200):
        pose = hm.draw_pose(np.random.default_rng(seed))
        J = hm.joints_model(pose)
        want = rest * pose['factor'][finger]
        for Jx in (J, J @ hm.global_rotation(pose).T):                      # the global rotation keeps them too
            got = np.array([np.linalg.norm(Jx[c] - Jx[p]) for p, c in HAND_BONES])
            assert np.abs(got - want).max() <= 1e-12, seed
    R3 = hm.global_rotation(hm.draw_pose(np.random.default_rng(0)))
    assert np.abs(R3 @ R3.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R3) - 1.0) < 1e-12


def test_every_drawn_angle_lies_in_its_range_over_2000_seeds():
    from utils import hand_model as hm
    lo = np.array([[r[0] for r in (hm.THUMB_FLEX if f == 0 else hm.FLEX)] for f in range(5)])
    hi = np.array([[r[1] for r in (hm.THUMB_FLEX if f == 0 else hm.FLEX)] for f in range(5)])
    alo = np.array([hm.THUMB_ABD[0]] + [hm.ABD_MCP[0]] * 4)
    ahi = np.array([hm.THUMB_ABD[1]] + [hm.ABD_MCP[1]] * 4)
    seen_flex_lo, seen_flex_hi = np.full((5, 3), np.inf), np.full((5, 3), -np.inf)
    for seed in range(2000):
        p = hm.draw_pose(np.random.default_rng(seed))
        assert ((p['flex'] >= lo) & (p['flex'] <= hi)).all() and ((p['abd'] >= alo) & (p['abd'] <= ahi)).all(), seed
        assert hm.FINGER_FACTOR[0] <= p['factor'].min() and p['factor'].max() <= hm.FINGER_FACTOR[1]
        assert 0.0 <= p['rotation'] < 360.0 and 0.0 <= p['tilt'] <= hm.TILT_MAX
        assert hm.SPAN_SHARE[0] <= p['span'] <= hm.SPAN_SHARE[1] and np.abs(p['shift']).max() <= hm.SHIFT_SHARE
        seen_flex_lo, seen_flex_hi = np.minimum(seen_flex_lo, p['flex']), np.maximum(seen_flex_hi, p['flex'])
    assert ((seen_flex_hi - seen_flex_lo) > 0.9 * (hi - lo)).all()           # ... and the ranges are used, thumb and fingers apart


def test_items_are_pure_functions_of_seed_index_domain_and_gap():
    a = _ds(domain='photo')
    r0, k0, v0 = a[5]
    r1, k1, v1 = a[5]
    assert r0.tobytes() == r1.tobytes() and np.array_equal(k0, k1) and np.array_equal(v0, v1)
    assert r0.dtype.itemsize == 480 and k0.shape == (21, 2) and k0.dtype == np.float32 and v0.shape == (21, 1)
    assert np.array_equal(k0[:, 0], r0['jx']) and np.array_equal(k0[:, 1], r0['jy'])      # the un-quantised joints of the record
    for other in (a[6], _ds(domain='cg')[5], _ds(domain='photo', seed=8)[5], _ds(domain='photo', gap=0.5)[5]):
        assert other[0].tobytes() != r0.tobytes() and not np.array_equal(other[1], k0)
    assert _ds(domain='cg', gap=0.0)[5][0].tobytes() == _ds(domain='cg', gap=1.0)[5][0].tobytes()      # gap does nothing to 'cg'
    assert a.num_keypoints == 21 and set(a.keypoints_group) == {'MCP', 'PIP', 'DIP', 'fingertip', 'all'}
    assert abs(a.group_accuracy(list(range(21)))['all'] - 10.0) < 1e-9
    with pytest.raises(ValueError):
        _ds(domain='real')
    with pytest.raises(ValueError):
        _ds(gap=1.5)


def test_gap_zero_photo_records_have_the_cg_style_distribution():
    from utils import rendered_dataset as D
    cg, p0, p1 = _ds(domain='cg'), _ds(domain='photo', gap=0.0), _ds(domain='photo', gap=1.0)
    n = 300
    rc, r0, r1 = (np.array([d[i][0] for i in range(n)]) for d in (cg, p0, p1))
    for r in (rc, r0):
        assert not r['occ_r'].any() and not r['sensor_sigma'].any() and not r['noise_amp'].any()
        assert (r['gain'] == 1.0).all() and (r['bias'] == 0.0).all()
        assert (r['ambient'] >= np.float32(D.AMBIENT[0][0])).all() and (r['ambient'] <= np.float32(D.AMBIENT[0][1])).all()
        assert (r['light'][:, 2] >= np.cos(np.deg2rad(D.LIGHT_ANGLE[0][1])) - 1e-6).all()
        assert (r['bg0'] <= D.BG_DARK[0][1] + 1e-6).all() and (r['bg1'] >= D.BG_BRIGHT[0][0] - 1e-6).all()
    assert abs(rc['ambient'].mean() - r0['ambient'].mean()) < 0.02 and abs(rc['skin'].mean() - r0['skin'].mean()) < 0.02
    # the full gap: every photo-only effect occurs, an occluder in roughly its stated share
    assert (r1['sensor_sigma'] > 0).all() and (r1['noise_amp'] > 0).all() and (r1['gain'] != 1.0).any() and (r1['bias'] != 0.0).any()
    assert 0.2 < (r1['occ_r'] > 0).mean() < 0.5
    assert np.allclose(np.linalg.norm(r1['light'], axis=1), 1.0, atol=1e-6)
    assert ((r1['noise_inv_cell'] > 0) & (r1['noise_inv_cell'] <= 1)).all()


def test_visible_is_one_iff_the_joint_is_inside_the_frame():
    d = _ds(domain='photo')
    S, out = 64, 0
    for i in range(300):
        _, kp, vis = d[i]
        inside = (kp[:, 0] >= -0.5) & (kp[:, 0] < S - 0.5) & (kp[:, 1] >= -0.5) & (kp[:, 1] < S - 0.5)
        assert np.array_equal(vis[:, 0] == 1.0, inside) and set(np.unique(vis)) <= {0.0, 1.0}
        out += int((~inside).sum())
    assert 0 < out < 0.2 * 300 * 21                                           # most joints in frame, some leave it


def test_record_dtype_mirrors_the_header_struct():
    import re
    import os
    from conftest import ROOT
    from mi355.ops import HAND_REC_DTYPE
    assert HAND_REC_DTYPE.itemsize % 16 == 0 and HAND_REC_DTYPE.itemsize == 480
    txt = open(os.path.join(ROOT, 'include', 'mi355pose.h')).read()
    body = re.search(r'typedef struct mi355_hand_rec \{(.*?)\} mi355_hand_rec;', txt, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for name in rest.split(','):
            m = re.match(r'\s*(\w+)(?:\[(\d+)\])?\s*$', name)
            fields.append((m.group(1), {'float': '<f4', 'uint32_t': '<u4'}[ctype], int(m.group(2) or 1)))
    mine = [(n, HAND_REC_DTYPE[n].base.str, int(np.prod(HAND_REC_DTYPE[n].shape or (1,)))) for n in HAND_REC_DTYPE.names]
    assert mine == fields
    assert [HAND_REC_DTYPE.fields[n][1] for n in HAND_REC_DTYPE.names] == list(np.cumsum([0] + [4 * c for _, _, c in fields[:-1]]))


def test_reference_render_covers_the_pixel_of_every_visible_joint():
    from uda.model.loss import HAND_BONES
    S = 32
    bones_of = {j: [b for b, (p, c) in enumerate(HAND_BONES) if j in (p, c)] for j in range(21)}
    grid = [a.astype(np.float32) for a in np.meshgrid(np.arange(S), np.arange(S))]
    checked = 0
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        for domain in ('cg', 'photo'):
            d = _ds(image_size=S, heatmap_size=8, domain=domain)
            for i in range(200):
                rec, kp, vis = d[i]
                rec = rec.copy()
                rec['occ_r'] = 0.0                                            # (an occluder covers pixels too: the hand alone must)
                ids = R.trace(R.primitives(rec), *grid)[0] + 1
                for j in range(21):
                    if vis[j, 0] and any(rec['radius'][b] > 0 for b in bones_of[j]):
                        assert 1 <= ids[int(kp[j, 1] + 0.5), int(kp[j, 0] + 0.5)] <= 20, (domain, i, j)
                        checked += 1
    assert checked > 0.9 * 2 * 200 * 21


def test_degenerate_primitives_cover_nothing_and_nothing_invalid_reaches_an_index():
    S = 32
    rec = _ds(image_size=S, heatmap_size=8, domain='photo')[2][0].copy()
    rec['occ_r'] = 0.0
    mean3, inv3 = R.norm()
    with warnings.catch_warnings():
        warnings.simplefilter('error')                                        # (numpy warns when an invalid value is cast to an integer)
        base = R.render(rec, S, mean3, inv3)
        z = rec.copy()                                                        # a zero-length bone: t = 0 by selection, a disc of its radius
        z['jx'][6], z['jy'][6], z['jz'][6] = z['jx'][5], z['jy'][5], z['jz'][5]
        out = R.render(z, S, mean3, inv3)
        assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
        r0 = rec.copy()                                                       # zero radius: bone 9 is gone, nothing else changes
        r0['radius'][9] = 0.0
        ids = R.render(r0, S, mean3, inv3)[2]
        assert not (ids == 10).any() and np.array_equal(ids[base[2] != 10], base[2][base[2] != 10])
        for bad in (np.nan, np.inf, -np.inf, 3.0e6):                          # a joint that is NaN, infinite or out of range: its bones are gone
            n = rec.copy()
            n['jx'][6] = bad
            out = R.render(n, S, mean3, inv3)
            assert np.isfinite(out[0]).all() and not np.isin(out[2], (6, 7)).any() and (out[2] == 5).any()
        e = rec.copy()                                                        # every primitive invalid: the background alone
        e['jz'][:] = np.nan
        out = R.render(e, S, mean3, inv3)
        assert not out[2].any() and np.isfinite(out[0]).all()
        w = rec.copy()                                                        # an invalid noise cell size switches the noise off, it is never floored
        for bad in (np.nan, np.inf, 0.0, -1.0, 2.0):
            w['noise_inv_cell'] = bad
            assert np.isfinite(R.render(w, S, mean3, inv3)[0]).all()


def test_image_ema_differs_from_the_image_only_by_gain_bias_and_sensor_noise():
    S = 32
    mean3, inv3 = R.norm()
    cg = _ds(image_size=S, heatmap_size=8, domain='cg')[0][0]
    out, ema, _ = R.render(cg, S, mean3, inv3)
    assert np.array_equal(out, ema)                                           # cg: gain 1, bias 0, no sensor noise -- m * 1 + 0 is m
    p = _ds(image_size=S, heatmap_size=8, domain='photo')[0][0].copy()
    out, ema, _ = R.render(p, S, mean3, inv3)
    assert not np.array_equal(out, ema)
    p['gain'], p['bias'], p['sensor_sigma'] = 1.0, 0.0, 0.0
    plain, ema2, _ = R.render(p, S, mean3, inv3)
    assert np.array_equal(ema, ema2)
    assert np.array_equal(plain, ema2)


def test_hash_is_uniform_enough_and_exactly_a_multiple_of_2_to_the_minus_24():
    i, j = np.meshgrid(np.arange(64, dtype=np.uint32), np.arange(64, dtype=np.uint32))
    u = R.hash01(np.uint32(12345), i, j)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))
    assert abs(u.mean() - 0.5) < 0.02 and abs(u.std() - 12 ** -0.5) < 0.02
    assert not np.array_equal(u, R.hash01(np.uint32(12346), i, j)) and not np.array_equal(u, u.T)


def test_parser_checks_of_the_rendered_flags(capsys):
    import train1
    p = train1.build_parser()
    a = p.parse_args(['d', '--synthetic-hands'])
    assert a.synthetic_hands and not a.synthetic and a.render_gap == 1.0 and a.render_train_size == 65536 and a.render_val_size == 512
    assert not p.parse_args(['d']).synthetic_hands
    for argv, words in ((['d', '--synthetic-hands', '--synthetic'], ('--synthetic', '--synthetic-hands')),
                        (['d', '--synthetic-hands', '--device-augment'], ('--device-augment', '--synthetic-hands')),
                        (['d', '--synthetic-hands', '--render-gap', '1.5'], ('--render-gap',)),
                        (['d', '--render-gap', '-0.1'], ('--render-gap',)),
                        (['d', '--synthetic-hands', '--render-gap', 'nan'], ('--render-gap',)),
                        (['d', '--synthetic-hands', '--image-size', '100'], ('--image-size',))):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
        err = capsys.readouterr().err
        assert all(w in err for w in words), (argv, err[-300:])
    ds = train1.build_datasets(p.parse_args(['d', '--synthetic-hands', '--image-size', '64', '--heatmap-size', '16', '--render-gap', '0.5',
                                             '--render-train-size', '32', '--render-val-size', '8']))
    assert [(len(d), d.domain, d.gap) for d in ds] == [(32, 'cg', 0.5), (8, 'cg', 0.5), (32, 'photo', 0.5), (8, 'photo', 0.5)]
    assert len({d.seed for d in ds}) == 4                                     # validation seeds disjoint from training


def test_record_collate_packs_one_buffer_per_batch():
    import torch
    from utils.data import record_collate
    d = _ds(domain='photo')
    items = [d[i] for i in range(3)]
    flat = record_collate(items)
    assert flat.dtype == torch.uint8 and flat.shape == (3 * (480 + 21 * 12),)
    raw = flat.numpy()
    assert raw[:3 * 480].tobytes() == b''.join(it[0].tobytes() for it in items)
    assert np.array_equal(raw[3 * 480:3 * 480 + 3 * 168].view(np.float32).reshape(3, 21, 2), np.stack([it[1] for it in items]))
    assert np.array_equal(raw[3 * 480 + 3 * 168:].view(np.float32).reshape(3, 21, 1), np.stack([it[2] for it in items]))
