"""A procedural articulated hand: the 21 joints and 20 bones of ``uda.model.loss.HAND_BONES`` posed from per-sample draws and
projected weak-perspectively to image pixels.  Host code, numpy float64 throughout; nothing here touches a GPU.

Model space: the wrist is the origin, the palm lies in the plane z = 0, +y points from the wrist to the middle finger's knuckle,
the unit of length is the distance between those two.  The camera looks along +z, so a smaller z is nearer and flexion (fingers
curling towards the palm side) moves a finger towards -z.  Finger f = 0 .. 4 (thumb .. little finger) owns joints 4f+1 .. 4f+4:
its base in the palm plane (CMC for the thumb, MCP otherwise), then the ends of its three phalanges."""
import numpy as np

from uda.model.loss import HAND_BONES

NUM_JOINTS = 21
NUM_BONES = len(HAND_BONES)

# ---- rest proportions (fixed) -------------------------------------------------------------------------------------------------
# bases in the palm plane: rough adult proportions, the knuckle arc falling away towards the little finger
REST_BASE = np.array([[-0.36, 0.26], [-0.25, 0.95], [0.0, 1.0], [0.22, 0.94], [0.42, 0.82]])
# direction of each finger at rest, degrees from +y towards +x: the fingers fan out, the thumb points away from the palm
REST_ANGLE = np.array([-52.0, -8.0, 0.0, 8.0, 18.0])
# phalanx lengths, proximal to distal: the middle finger about as long as the palm, each phalanx ~0.6-0.75 of the one before
REST_PHALANX = np.array([[0.42, 0.32, 0.28], [0.45, 0.27, 0.22], [0.50, 0.30, 0.23], [0.46, 0.28, 0.22], [0.36, 0.21, 0.20]])
# wrist to middle fingertip at rest: the "span" a scale is stated against
REST_SPAN = 1.0 + float(REST_PHALANX[2].sum())
# bone radii in model units: [finger][wrist->base, proximal, middle, distal]; the wrist->base capsules are about as fat as the
# knuckles are apart (0.22 .. 0.25), so the five of them merge into one palm
REST_RADIUS = np.array([[0.17, 0.105, 0.095, 0.085], [0.21, 0.085, 0.075, 0.065], [0.21, 0.088, 0.078, 0.068],
                        [0.21, 0.083, 0.073, 0.063], [0.20, 0.072, 0.064, 0.056]])
# no bone is drawn thinner than this many pixels: more than half a pixel diagonal, so the pixel a joint rounds to is always covered
MIN_RADIUS_PX = 0.75

# ---- per-sample ranges ----------------------------------------------------------------------------------------------------------
FINGER_FACTOR = (0.88, 1.12)        # per-finger length factor: the spread of finger-to-palm ratios between people
FLEX_MCP = (-10.0, 80.0)            # degrees; a knuckle hyper-extends a little and flexes to about a right angle
FLEX_PIP = (0.0, 100.0)             # the middle joint does not hyper-extend and flexes the furthest
FLEX_DIP = (0.0, 70.0)              # the end joint flexes less than the middle one
ABD_MCP = (-12.0, 12.0)             # sideways spread of a finger at its knuckle
THUMB_FLEX_CMC = (-10.0, 45.0)      # the thumb's saddle joint moves less towards the palm than a knuckle
THUMB_FLEX_MCP = (0.0, 50.0)        # about half of a finger's middle joint
THUMB_FLEX_IP = (-5.0, 70.0)        # the thumb's end joint hyper-extends slightly
THUMB_ABD = (-20.0, 25.0)           # the thumb swings towards and away from the index finger further than a finger spreads
ROTATION = (0.0, 360.0)             # in-plane rotation: a hand is seen at any angle
TILT_MAX = 40.0                     # out-of-plane tilt, degrees: beyond it the weak-perspective silhouette stops looking like a hand
SPAN_SHARE = (0.45, 0.75)           # wrist-to-fingertip rest span as a share of the image side (hand crops are scaled about so)
SHIFT_SHARE = 0.30                  # the hand's centre lies within this share of the side from the image centre, per axis: at
                                    # the largest span most joints stay in frame and the outermost can leave it

FLEX = (FLEX_MCP, FLEX_PIP, FLEX_DIP)
THUMB_FLEX = (THUMB_FLEX_CMC, THUMB_FLEX_MCP, THUMB_FLEX_IP)


def _uniform(rng, lohi, size=None):
    return rng.uniform(lohi[0], lohi[1], size)


def draw_pose(rng):
    """The per-sample draws, angles in degrees: factor (5,), flex (5, 3), abd (5,), rotation, tilt, tilt_axis, span share,
    shift (2,) as shares of the side.  Always the same number of draws from `rng`."""
    flex = np.empty((5, 3))
    abd = np.empty(5)
    for f in range(5):
        for k, r in enumerate(THUMB_FLEX if f == 0 else FLEX):
            flex[f, k] = _uniform(rng, r)
        abd[f] = _uniform(rng, THUMB_ABD if f == 0 else ABD_MCP)
    return dict(factor=_uniform(rng, FINGER_FACTOR, 5), flex=flex, abd=abd, rotation=_uniform(rng, ROTATION),
                tilt=_uniform(rng, (0.0, TILT_MAX)), tilt_axis=_uniform(rng, (0.0, 360.0)), span=_uniform(rng, SPAN_SHARE),
                shift=_uniform(rng, (-SHIFT_SHARE, SHIFT_SHARE), 2))


def joints_model(pose):
    """(21, 3) joints in model units, before the global rotation: every bone of finger f has its rest length times factor[f]."""
    J = np.zeros((NUM_JOINTS, 3))
    for f in range(5):
        k = pose['factor'][f]
        a = np.deg2rad(REST_ANGLE[f] + pose['abd'][f])
        d = np.array([np.sin(a), np.cos(a), 0.0])
        p = np.array([REST_BASE[f, 0], REST_BASE[f, 1], 0.0]) * k
        J[4 * f + 1] = p
        phi = 0.0
        for s in range(3):
            phi += np.deg2rad(pose['flex'][f, s])
            p = p + REST_PHALANX[f, s] * k * (np.cos(phi) * d + np.sin(phi) * np.array([0.0, 0.0, -1.0]))
            J[4 * f + 2 + s] = p
    return J


def rest_lengths():
    """(20,) rest length of every bone of HAND_BONES, model units."""
    out = np.empty(NUM_BONES)
    for b, (p, c) in enumerate(HAND_BONES):
        f, s = (c - 1) // 4, (c - 1) % 4
        out[b] = np.hypot(*REST_BASE[f]) if s == 0 else REST_PHALANX[f, s - 1]
    return out


def bone_finger():
    """(20,) the finger every bone belongs to."""
    return np.array([(c - 1) // 4 for _, c in HAND_BONES])


def global_rotation(pose):
    """3 x 3: a tilt about an axis in the palm plane, then the in-plane rotation."""
    t, ax, r = np.deg2rad(pose['tilt']), np.deg2rad(pose['tilt_axis']), np.deg2rad(pose['rotation'])
    u = np.array([np.cos(ax), np.sin(ax), 0.0])
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    tilt = np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)
    rz = np.array([[np.cos(r), -np.sin(r), 0.0], [np.sin(r), np.cos(r), 0.0], [0.0, 0.0, 1.0]])
    return rz @ tilt


def project(pose, side):
    """Weak perspective to an image of `side` pixels: (21, 3) pixel x, y and a depth z in pixels (smaller is nearer), the 20 bone
    radii in pixels, and the pixels-per-unit scale."""
    J = joints_model(pose) @ global_rotation(pose).T
    scale = pose['span'] * side / REST_SPAN
    P = J * scale
    centre = (side - 1) / 2.0 + pose['shift'] * side
    P[:, :2] += centre - P[:, :2].mean(axis=0)
    radius = np.array([REST_RADIUS[(c - 1) // 4, (c - 1) % 4] * pose['factor'][(c - 1) // 4] for _, c in HAND_BONES]) * scale
    return P, np.maximum(radius, MIN_RADIUS_PX), scale
