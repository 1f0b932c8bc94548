"""CPU: the registration metrics of roitr_amd/registration.py (registration/benchmark.py restated) against numpy restatements
written here, and the 3DMatch .log / .info text format.  Imports only: no GPU is touched."""
import numpy as np
import pytest
import torch


def rot_from_quat(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_from_rot(R):
    """w >= 0 quaternion of a rotation by Shepperd's branch rule (an independent form of nibabel's mat2quat)."""
    tr = np.trace(R)
    if tr > 0:
        S = np.sqrt(tr + 1.0) * 2
        q = np.array([0.25 * S, (R[2, 1] - R[1, 2]) / S, (R[0, 2] - R[2, 0]) / S, (R[1, 0] - R[0, 1]) / S])
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        S = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = np.array([(R[2, 1] - R[1, 2]) / S, 0.25 * S, (R[0, 1] + R[1, 0]) / S, (R[0, 2] + R[2, 0]) / S])
    elif R[1, 1] > R[2, 2]:
        S = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = np.array([(R[0, 2] - R[2, 0]) / S, (R[0, 1] + R[1, 0]) / S, 0.25 * S, (R[1, 2] + R[2, 1]) / S])
    else:
        S = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = np.array([(R[1, 0] - R[0, 1]) / S, (R[0, 2] + R[2, 0]) / S, (R[1, 2] + R[2, 1]) / S, 0.25 * S])
    return -q if q[0] < 0 else q


def test_rotation_and_translation_error():
    from roitr_amd.registration import rotation_error, translation_error
    rng = np.random.default_rng(0)
    R1 = np.stack([rot_from_quat(rng.normal(size=4)) for _ in range(6)])
    R2 = np.stack([rot_from_quat(rng.normal(size=4)) for _ in range(6)])
    R2[0] = R1[0]                                # 0 degrees (trace term clamped at 1)
    R2[1] = R1[1] @ rot_from_quat(np.array([0.0, 0, 0, 1]))   # 180 degrees
    got = rotation_error(torch.from_numpy(R1), torch.from_numpy(R2)).numpy()
    ref = np.degrees(np.arccos(np.clip((np.einsum("bji,bji->b", R1, R2) - 1) / 2, -1, 1)))
    assert got.shape == (6, 1) and np.abs(got[:, 0] - ref).max() < 1e-9
    assert abs(got[0, 0]) < 1e-5 and abs(got[1, 0] - 180) < 1e-5
    t1, t2 = rng.normal(size=(6, 3, 1)), rng.normal(size=(6, 3, 1))
    assert np.abs(translation_error(torch.from_numpy(t1), torch.from_numpy(t2)).numpy() - np.linalg.norm((t1 - t2)[..., 0], axis=1)).max() < 1e-12


@pytest.mark.parametrize("seed", range(6))
def test_compute_transformation_err(seed):
    from roitr_amd.registration import _mat2quat, compute_transformation_err
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    if seed == 0:
        q = np.array([0.0, 1.0, 0.0, 0.0])      # w = 0: the sign rule decides
    R = rot_from_quat(q)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, rng.normal(size=3)
    A = rng.normal(size=(6, 6))
    info = A @ A.T + 6 * np.eye(6)
    qq = quat_from_rot(R)
    mq = _mat2quat(R)
    if abs(qq[0]) > 1e-9:
        assert np.abs(mq - qq).max() < 1e-9
    else:   # w = 0: q and -q both have w >= 0
        assert min(np.abs(mq - qq).max(), np.abs(mq + qq).max()) < 1e-9
    er = np.concatenate([T[:3, 3], mq[1:]])
    assert abs(compute_transformation_err(T, info) - er @ info @ er / info[0, 0]) < 1e-9 * max(1.0, er @ info @ er)
    er = np.concatenate([T[:3, 3], qq[1:]])
    if abs(qq[0]) > 1e-9:
        assert abs(compute_transformation_err(T, info) - er @ info @ er / info[0, 0]) < 1e-9 * max(1.0, er @ info @ er)


def _trajectories(rng, num_fragment=8):
    pairs, gt = [], []
    for i in range(num_fragment):
        for j in range(i + 1, num_fragment):
            pairs.append([i, j, num_fragment])
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = rot_from_quat(rng.normal(size=4)), rng.normal(size=3)
            gt.append(T)
    return np.array(pairs), np.array(gt)


def test_evaluate_registration_rules():
    from roitr_amd.registration import compute_transformation_err, evaluate_registration
    rng = np.random.default_rng(3)
    pairs, gt = _trajectories(rng)
    info = np.tile(np.eye(6), (len(pairs), 1, 1))
    est = gt.copy()
    # non-consecutive pairs only; gt index 0 is never tested (the reference's mask uses 0 for "absent")
    tested = [k for k in range(len(pairs)) if pairs[k, 1] - pairs[k, 0] > 1 and k > 0]
    # perturb translations to land just inside / just outside the 0.2 m RMSE (info = I: p = |t_err|^2)
    inside, outside = tested[0], tested[1]
    est[inside][:3, 3] += gt[inside][:3, :3] @ np.array([0.199, 0, 0])
    est[outside][:3, 3] += gt[outside][:3, :3] @ np.array([0.201, 0, 0])
    consecutive = [k for k in range(len(pairs)) if pairs[k, 1] - pairs[k, 0] == 1][0]
    est[consecutive][:3, 3] += 5.0     # not tested, cannot lower the recall
    prec, rec, flags = evaluate_registration(8, est, pairs, pairs, gt, info)
    assert flags[outside] == 1 and flags[inside] == 0 and flags[consecutive] == 2
    assert all(flags[k] == 2 for k in range(len(pairs)) if k not in tested)
    assert abs(rec - (len(tested) - 1) / len(tested)) < 1e-12 and abs(prec - (len(tested) - 1) / len(tested)) < 1e-12
    p_in = compute_transformation_err(np.linalg.inv(gt[inside]) @ est[inside], info[inside])
    assert abs(p_in - 0.199 ** 2) < 1e-9
    # a stricter threshold moves the inside pair out
    _, rec2, flags2 = evaluate_registration(8, est, pairs, pairs, gt, info, err2=0.19)
    assert flags2[inside] == 1 and rec2 < rec


def test_log_and_info_round_trip(tmp_path):
    from roitr_amd.registration import read_trajectory, read_trajectory_info, write_trajectory, write_trajectory_info
    rng = np.random.default_rng(4)
    pairs, traj = _trajectories(rng, 5)
    write_trajectory(traj, pairs, str(tmp_path / "est.log"))
    keys, back = read_trajectory(str(tmp_path / "est.log"))
    assert np.array_equal(keys.astype(int), pairs) and np.abs(back - traj).max() < 1e-11
    meta = pairs.copy()
    meta[2, 2] = 0      # write_trajectory skips pairs whose third metadata field is 0
    write_trajectory(traj, meta, str(tmp_path / "skip.log"))
    keys2, back2 = read_trajectory(str(tmp_path / "skip.log"))
    assert len(keys2) == len(pairs) - 1 and np.abs(back2 - np.delete(traj, 2, 0)).max() < 1e-11
    A = rng.normal(size=(len(pairs), 6, 6))
    info = A @ np.transpose(A, (0, 2, 1))
    write_trajectory_info(info, pairs, str(tmp_path / "gt.info"))
    n_frame, info_back = read_trajectory_info(str(tmp_path / "gt.info"))
    assert n_frame == 5 and np.abs(info_back - info).max() < 1e-11
