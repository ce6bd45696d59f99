"""The numpy reference of the fit report (tests/fit_report_ref.py) on hand-made maps with known answers, and the caps on the
inputs the GPU tests run the vertex kernel on: at most 1 % undecided vertices, both kinds of decided vertices present."""
import numpy as np
import pytest

import fit_report_ref as fr


def _maps(T, H, W):
    return np.full((T, H, W), -1, np.int32), np.full((T, H, W), -1.0, np.float32), np.zeros((T, H, W), np.uint32)


def test_rendered_region_equal_to_its_mask_has_iou_one():
    person, depth, bits = _maps(1, 8, 10)
    person[0, 2:6, 3:7] = 0
    depth[0, 2:6, 3:7] = 3.0
    bits[0, 2:6, 3:7] = 1
    counts, dsum = fr.pixels_ref(person, depth, bits, 1)
    assert counts[0, 0].tolist() == [16, 16, 16, 0] and (dsum == 0).all()
    iou, bias, absd = fr.derived_ref(counts, dsum)
    assert iou[0, 0] == 1.0


def test_mask_shifted_by_two_columns():
    person, depth, bits = _maps(1, 8, 10)
    person[0, 2:6, 3:7] = 0
    depth[0, 2:6, 3:7] = 3.0
    bits[0, 2:6, 5:9] = 1
    # target depth: disp 0.5 between min_z 1 and max_z 3 -> 1 / (0.5 (1 - 1/3) + 1/3) = 1.5 m; d = 3 + 0.2 - 1.5
    disp = np.full((1, 8, 10), 0.5, np.float32)
    scene_depth = np.full((8, 10), 2.5, np.float32)
    scene_mask = np.zeros((8, 10), np.uint8)
    scene_mask[:, :5] = 1
    counts, dsum = fr.pixels_ref(person, depth, bits, 1, disp=disp, min_z=[1.0], max_z=[3.0], scene_depth=scene_depth,
                                 scene_mask=scene_mask)
    assert counts[0, 0].tolist() == [16, 16, 8, 8]          # behind: the rendered columns 3 and 4, 3.0 > 2.5 + 0.05
    iou, bias, absd = fr.derived_ref(counts, dsum)
    assert iou[0, 0] == pytest.approx(8 / 24)
    assert bias[0, 0] == pytest.approx(1.7, abs=1e-6) and absd[0, 0] == pytest.approx(1.7, abs=1e-6)
    # the comparison with the surface is a float32 one: a pixel exactly on scene_depth + margin is not behind it
    depth[0, 2:6, 3:5] = np.float32(2.5) + np.float32(0.05)
    assert fr.pixels_ref(person, depth, bits, 1, scene_depth=scene_depth, scene_mask=scene_mask)[0][0, 0, 3] == 0


def test_person_without_a_rendered_pixel():
    person, depth, bits = _maps(2, 6, 6)
    bits[:, 1:3, 1:3] = 2                      # person 1 is segmented, never rendered
    person[0, 4, 4] = 0
    counts, dsum = fr.pixels_ref(person, depth, bits, 2, disp=np.ones((2, 6, 6), np.float32), min_z=[1, 1], max_z=[3, 3])
    assert counts[:, 1].tolist() == [[0, 4, 0, 0], [0, 4, 0, 0]] and counts[0, 0].tolist() == [1, 0, 0, 0]
    iou, bias, absd = fr.derived_ref(counts, dsum)
    assert iou[0, 1] == 0.0 and np.isnan(bias[0, 1]) and np.isnan(absd[1, 1])
    assert np.isnan(iou[1, 0])                 # neither rendered nor segmented: no union


def test_bit_31_is_person_31():
    person, depth, bits = _maps(1, 4, 4)
    bits[0, 0, :3] = np.uint32(1) << np.uint32(31)
    person[0, 0, 1:4] = 31
    for words in (bits, bits.view(np.int32)):              # the words may arrive signed: the sign bit is a person
        counts, _ = fr.pixels_ref(person, depth, words, 32)
        assert counts[0, 31].tolist() == [3, 3, 2, 0] and counts[0, :31].sum() == 0


def test_float32_and_float64_sums_differ_but_little():
    cases = [fr.pixel_case(*s) for s in fr.PIXEL_SHAPES]
    budget = fr.sum_budget(cases)
    print('largest float32 error of a sum relative to sum |d|: %.3e' % budget)
    assert 0 < budget < 1e-5


@pytest.mark.parametrize('shape', fr.PIXEL_SHAPES)
def test_pixel_cases_exercise_every_count(shape):
    c = fr.pixel_case(*shape)
    counts, dsum = fr.pixels_ref(c['person'], c['depth'], c['bits'], c['N'], disp=c['disp'], min_z=c['min_z'], max_z=c['max_z'],
                                 scene_depth=c['scene_depth'], scene_mask=c['scene_mask'])
    assert (counts[..., 2] <= np.minimum(counts[..., 0], counts[..., 1])).all()
    # (the last shape has one frame without a rendered pixel and one without a mask: no intersection at all)
    assert (counts[..., 2].sum() > 0) == (shape[2:] != (135, 240))
    if shape[1] == 32:
        assert (counts[..., :3] > 0).all()                 # every person present, bit 31 included
    if shape[2:] == (135, 240):
        assert counts[0, :, 0].sum() == 0 and counts[1, :, 1].sum() == 0
        assert counts[1, :, 0].sum() > 0 and counts[0, :, 1].sum() > 0
    if shape != (1, 1, 1, 1):
        assert counts[..., 3].sum() > 0 and (counts[..., 3] < counts[..., 0]).any()


@pytest.mark.parametrize('name', fr.VERTEX_CASES)
def test_vertex_cases_keep_the_caps(name):
    c = fr.vertex_case(name)
    ref = fr.verts_ref(c['verts'], c['K'], c['scene_depth'], c['scene_mask'], c['margin'])
    total = c['B'] * c['V']
    und, ins, outs = int(ref['undecided'].sum()), int(ref['inside'].sum()), int(ref['outside'].sum())
    print('%s: %d vertices, %d undecided (%.2f %%), %d decided inside, %d decided outside' % (name, total, und, 100.0 * und / total,
                                                                                          ins, outs))
    assert und <= 0.01 * total                             # the cap: a case above it gets another seed, not another cap
    if name in fr.STATISTICAL:
        assert ins >= 20 and outs >= 20                    # a kernel that counts nothing, or everything, fails
        z = c['verts'][..., 2]
        assert (z <= 0).any() and (z > 0).any()
    if name == 'one':
        assert ins == 1
    if name == 'five':
        assert ins == 1 and outs == 1
    if name in ('zero_mask', 'none_inside'):
        assert ins == 0
    if name == 'none_inside':
        assert outs >= 20


def test_check_verts_accepts_the_reference_and_rejects_a_miscount():
    c = fr.vertex_case('small')
    ref = fr.verts_ref(c['verts'], c['K'], c['scene_depth'], c['scene_mask'], c['margin'])
    n = ref['inside'].sum(-1)
    m = np.float32([ref['pen'][b][ref['inside'][b]].max() if n[b] else 0 for b in range(c['B'])])
    fr.check_verts(ref, n, m)
    with pytest.raises(AssertionError):
        fr.check_verts(ref, n - 1, m)
    with pytest.raises(AssertionError):
        fr.check_verts(ref, n, np.nextafter(m, np.float32(10)))


def test_derived_columns_of_the_reference():
    K = np.float32([[100, 0, 50], [0, 100, 30], [0, 0, 1]])
    joints = np.float64([[[0.0, 0.0, 2.0], [0.2, 0.0, 2.0], [0.0, 0.2, 2.0]]])
    pose2d = np.float64([[[50, 30, 0.9], [63, 34, 0.9], [0, 0, 0.1]]])           # second joint: (60, 30) against (63, 34) = 5 px
    mean, worst, used = fr.reproj_ref(joints, K, None, pose2d, 0.5)
    assert mean[0] == pytest.approx(2.5) and worst[0] == pytest.approx(5.0) and used[0] == 2
    mean, worst, used = fr.reproj_ref(joints, K, None, pose2d, 0.95)
    assert np.isnan(mean[0]) and np.isnan(worst[0]) and used[0] == 0
    verts = np.float32([[[0, 1, 3], [0, 2, 3], [1, 2, 3]]])                      # lowest = largest y, first index on ties
    idx, low = fr.lowest_ref(verts)
    assert idx[0] == 1 and low[0].tolist() == [0, 2, 3]
    cloud = np.float32([[0, 2.5, 3]] * 40 + [[9, 9, 9]] * 5)
    assert fr.contact_ref(verts, cloud)[0] == pytest.approx(0.5)
    assert fr.foot_slide_ref(verts, verts + np.float32([0.3, 0, 0.4]))[0] == pytest.approx(0.5)
