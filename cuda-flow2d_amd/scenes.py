"""Seeded frame pairs with analytic ground-truth flow, for accuracy measurements (tools/accuracy_table.py, the flow-error tests).

Every frame is sampled exactly -- in double, stored float32 -- from a smooth analytic texture, a sum of sinusoids like
oracle.synthetic_pair's, at the inverse-mapped coordinates.  With the project's convention (flow2d_consistency_2d) the
ground truth w of frame 0 satisfies  I1(x + w(x)) = I0(x)  at every pixel x that is not occluded.

Scenes (make_scene(name, width, height, seed)):
  translation  a sub-pixel translation
  rotation     a rotation about the centre
  zoom         a zoom about the centre
  affine       a general affine motion
  two_layer    a textured square moving over a static textured background, with the exact occlusion map of frame 0: the
               background pixels the square covers in frame 1, and the square's pixels that leave the frame

Each Scene carries frame_0, frame_1, gt_u, gt_v (float32, height x width), occlusion (float32 0 / 1, or None where the scene
has no occlusion) and frame_1_at(x, y): the analytic frame 1 at any real coordinates (double), for checking the ground truth.
For frame interpolation (flow2d_interpolate_2d) it also carries gt_back_u, gt_back_v -- the true flow of frame 1 to frame 0,
I0(y + w_b(y)) = I1(y) at every pixel y of frame 1 that is not occluded --, occlusion_1 (frame 1's occlusion map, None where
the scene has none), frame_0_at(x, y) (the analytic frame 0), back_flow_at(x, y) (the backward flow at any real coordinates,
double) and frame_at_time(t): the exact frame at time t, 0 <= t <= 1, on
the linear trajectories x + t * w(x) (frame_0 at t = 0, frame_1 at t = 1).
Sequences (make_sequence(name, frame_count, width, height, seed)), for point tracking (flow2d_track_points_2d): the same scenes
carried on for frame_count frames with the same textures (frames 0 and 1 are make_scene's).  Affine scenes: frame k is the
texture at W^-k(x), W the scene's motion; two_layer: the square has moved by k * t in frame k.  Each Sequence carries frames
[frame_count, h, w], the true flows of every pair k -- gt_u[k], gt_v[k] (frame k -> k+1) and gt_back_u[k], gt_back_v[k]
(frame k+1 -> k) --, frame_at(k, x, y) (the analytic frame k, double), trajectory(x, y, k, start=0) (where the point at (x, y)
in frame `start` is in frame k, double) and visible(x, y, k, start=0): whether that point is seen in frame k (affine scenes:
inside the frame; two_layer: a background point is hidden while the square covers it, a square point is lost once it has left
the frame).  For temporal denoising (flow2d_denoise_2d) the same between any two frames, backwards too:
trajectory_between(x, y, start, k), visible_between(x, y, start, k) and flow_between(start, k) -> (u, v, visible) on frame
`start`'s grid.
Speckle scenes (make_speckle_scene(motion, width, height, seed), motion one of SPECKLE_MOTIONS), for window correlation
(flow2d_correlate_2d): the affine scenes' machinery on a Speckle texture, a seeded sum of Gaussian blobs as sprayed on a specimen
for digital image correlation -- fine, aperiodic detail in every window, which the long sinusoids of Texture do not have.  They
are NOT in SCENES: the tables and tests that iterate over that tuple are about the variational flow.
Speckle deformations (make_speckle_deformation(name, width, height, seed), name one of SPECKLE_DEFORMATIONS), for the subset
refinement (flow2d_subset_refine_2d): the same texture under a rotation, a stretch and a shear, each with a translation.
make_speckle_deformation_sequence(name, steps, step_size, ...) carries one of them on, k times per step k, every frame against
frame 0: the loading sequence flow2d_subset_refine_from_2d is for.  make_speckle_specimen(name, width, height, seed) puts the
same deformations on a plate with a hole in front of a static background and returns the scene with its mask: what
flow2d_subset_refine_masked_2d is for.  make_speckle_patchy(name, width, height, seed) puts them on a pattern whose contrast
varies by a decade from one 16-pixel patch to the next, so that the nodes' uncertainties do: what
flow2d_node_strain_weighted_2d is for.
Pure numpy: no device, no library.
"""
import numpy as np

SCENES = ("translation", "rotation", "zoom", "affine", "two_layer")


class Texture:
    """128 + sum of three sinusoids with seeded phases and orientations; smooth, with gradients in every direction."""

    def __init__(self, rng, amplitude=(55.0, 30.0, 18.0), periods=(61.0, 23.7, 37.3)):
        self.terms = []
        for a, p in zip(amplitude, periods):
            theta = rng.uniform(0, np.pi)
            self.terms.append((a, 2 * np.pi * np.cos(theta) / p, 2 * np.pi * np.sin(theta) / p, rng.uniform(0, 2 * np.pi)))

    def __call__(self, x, y):
        out = np.full(np.broadcast(x, y).shape, 128.0)
        for a, kx, ky, phase in self.terms:
            out += a * np.sin(kx * x + ky * y + phase)
        return out


SPECKLE_MOTIONS = ("translation", "affine", "large_translation")


class Speckle:
    """A dark ground plus one Gaussian blob per cell of a `pitch`-pixel grid, on the whole plane: the blob of cell (i, j) has its
    centre at a seeded position inside the cell and a seeded amplitude, both drawn from a hash of (i, j, seed), so nothing is
    stored and any real coordinate can be sampled.  A sample sums the blobs of the (2 * reach + 1)^2 cells around its own: the
    nearest blob left out is reach * pitch = 12 pixels = 8 sigma away, below 1e-11 grey levels."""

    def __init__(self, seed, pitch=4.0, sigma=1.5, ground=20.0, amplitude=(20.0, 110.0), reach=3):
        self.seed, self.pitch, self.sigma, self.ground, self.amplitude, self.reach = int(seed), pitch, sigma, ground, amplitude, reach

    def _uniform(self, i, j, stream):
        """[0, 1) from the cell and the stream number: the splitmix64 finaliser of a linear combination (wrapping uint64)."""
        with np.errstate(over="ignore"):
            z = (i.astype(np.int64).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) +
                 j.astype(np.int64).astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F) +
                 np.uint64((self.seed * 3 + stream) * 0x165667B19E3779F9 % 2 ** 64))
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53

    def __call__(self, x, y):
        x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
        ci, cj = np.floor(x / self.pitch), np.floor(y / self.pitch)
        out = np.full(x.shape, self.ground)
        lo, hi = self.amplitude
        for dj in range(-self.reach, self.reach + 1):
            for di in range(-self.reach, self.reach + 1):
                i, j = ci + di, cj + dj
                bx = (i + self._uniform(i, j, 0)) * self.pitch
                by = (j + self._uniform(i, j, 1)) * self.pitch
                amp = lo + (hi - lo) * self._uniform(i, j, 2)
                out += amp * np.exp(-((x - bx) ** 2 + (y - by) ** 2) / (2.0 * self.sigma ** 2))
        return out


def make_speckle_scene(motion, width=96, height=80, seed=0):
    """A speckle pattern under `motion` (one of SPECKLE_MOTIONS): the translation and the affine motion of make_scene, and a
    translation by (11.25, -7.5) -- almost three blob spacings, and more than a coarse-to-fine solver's finest levels reach."""
    texture = Speckle(seed)
    if motion == "translation":
        return _affine_scene("speckle_translation", width, height, texture, np.eye(2), (2.3, -1.4))
    if motion == "affine":
        return _affine_scene("speckle_affine", width, height, texture, [[1.02, 0.03], [-0.02, 0.985]], (1.25, -0.6))
    if motion == "large_translation":
        return _affine_scene("speckle_large_translation", width, height, texture, np.eye(2), (11.25, -7.5))
    raise ValueError("unknown speckle motion %r (one of %s)" % (motion, ", ".join(SPECKLE_MOTIONS)))


SPECKLE_DEFORMATIONS = ("rotation", "stretch", "shear")


def make_speckle_deformation(name, width=96, height=80, seed=0, translation=(1.6, -0.7)):
    """A speckle pattern whose windows deform (one of SPECKLE_DEFORMATIONS), for the subset refinement (flow2d_subset_refine_2d):
    a rotation by 5 degrees, a stretch by 1.06 x 0.97 and a shear of 0.08, each about the centre and followed by `translation`,
    (1.6, -0.7) by default.  They are NOT in SPECKLE_MOTIONS: the tests that iterate over that tuple are about the rigid window."""
    return _affine_scene("speckle_" + name, width, height, Speckle(seed), _speckle_deformation_matrix(name),
                         (float(translation[0]), float(translation[1])))


def _speckle_deformation_matrix(name):
    if name == "rotation":
        phi = np.radians(5.0)
        return [[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]]
    if name == "stretch":
        return [[1.06, 0.0], [0.0, 0.97]]
    if name == "shear":
        return [[1.0, 0.08], [0.0, 1.0]]
    raise ValueError("unknown speckle deformation %r (one of %s)" % (name, ", ".join(SPECKLE_DEFORMATIONS)))


class PatchySpeckle(Speckle):
    """Speckle whose contrast varies patchwise: over the ground, the blobs of the `patch`-pixel cell (i, j) are scaled by a seeded
    gain, log-uniform over `gain` = (0.1, 1) by default, from the same hash (stream 5).  A subset's displacement noise goes with
    noise / contrast, so that nodes on neighbouring patches differ in sigma by up to a decade: what a weighted strain window
    (flow2d_node_strain_weighted_2d) is for.  The gain belongs to the material and moves with it."""

    def __init__(self, seed, patch=16.0, gain=(0.1, 1.0), **speckle):
        super().__init__(seed, **speckle)
        self.patch, self.gain = float(patch), (float(gain[0]), float(gain[1]))

    def gain_at(self, x, y):
        x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
        lo, hi = self.gain
        return lo * (hi / lo) ** self._uniform(np.floor(x / self.patch), np.floor(y / self.patch), 5)

    def __call__(self, x, y):
        return self.ground + self.gain_at(x, y) * (super().__call__(x, y) - self.ground)


def make_speckle_patchy(name, width=96, height=80, seed=0, translation=(1.6, -0.7), patch=16.0, gain=(0.1, 1.0)):
    """make_speckle_deformation on a PatchySpeckle: the same motions and ground truth, the pattern's contrast varying by `gain` from
    one `patch`-pixel cell to the next.  With the grid of radius 7 and spacing 8 every other node's subset lies inside one cell."""
    return _affine_scene("patchy_" + name, width, height, PatchySpeckle(seed, patch, gain), _speckle_deformation_matrix(name),
                         (float(translation[0]), float(translation[1])))


def make_speckle_specimen(name, width=96, height=80, seed=0, translation=(1.6, -0.7), background_gain=0.3, background_offset=5.0):
    """A specimen in front of a background that does not move with it, for the masked subset refinement
    (flow2d_subset_refine_masked_2d): the deformation `name` (one of SPECKLE_DEFORMATIONS) of make_speckle_deformation, W about
    the centre c = ((width - 1) / 2, (height - 1) / 2), applied to a plate with a hole.  A point is *inside* when |x - c0| <=
    30.5 width / 96, |y - c1| <= 24.5 height / 80 and (x - c0)^2 + (y - c1)^2 > (9.5 min(width / 96, height / 80))^2.  T =
    Speckle(seed) is the specimen's texture, B = background_gain Speckle(seed + 7) + background_offset the static background
    (0.3 and 5 by default: dim; 1 and 0 give it the specimen's own contrast):
      frame_0(x) = inside(x) ? T(x) : B(x);   frame_1(X) = inside(W^-1 X) ? T(W^-1 X) : B(X).
    `translation` is the one W ends with, (1.6, -0.7) by default: a larger one moves the plate further than a window search's
    edge nodes can follow while their windows are half background (flow2d_correlate_masked_2d).
    Returns (scene, mask): the Scene of make_speckle_deformation with these frames (float32; gt_u, gt_v are W(x) - x everywhere,
    true on the specimen) and the mask in frame 0's coordinates, float32, 1 where not inside, else 0."""
    plain = make_speckle_deformation(name, width, height, seed, translation)
    texture, background = Speckle(seed), Speckle(seed + 7)
    background_gain, background_offset = float(background_gain), float(background_offset)
    c0, c1 = (width - 1) / 2.0, (height - 1) / 2.0
    half_w, half_h, hole = 30.5 * width / 96.0, 24.5 * height / 80.0, 9.5 * min(width / 96.0, height / 80.0)

    def inside(x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return (np.abs(x - c0) <= half_w) & (np.abs(y - c1) <= half_h) & ((x - c0) ** 2 + (y - c1) ** 2 > hole ** 2)

    def ground(x, y):
        return background_gain * background(x, y) + background_offset

    def frame_0_at(x, y):
        return np.where(inside(x, y), texture(x, y), ground(x, y))

    def frame_1_at(x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        bu, bv = plain.back_flow_at(x, y)
        return np.where(inside(x + bu, y + bv), texture(x + bu, y + bv), ground(x, y))

    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
    scene = Scene("specimen_" + name, frame_0_at(xs, ys).astype(np.float32), frame_1_at(xs, ys).astype(np.float32), plain.gt_u, plain.gt_v,
                  None, frame_1_at, frame_0_at=frame_0_at, back_flow_at=plain.back_flow_at)
    return scene, np.where(inside(xs, ys), 0.0, 1.0).astype(np.float32)


SPECKLE_BENDINGS = ("bend", "bulge")


def make_speckle_bending(name, width=96, height=80, seed=0, kappa=0.004):
    """A speckle pattern whose windows bend (one of SPECKLE_BENDINGS), for the second-order subset refinement
    (flow2d_subset_refine2_2d): frame_0 = T(x, y) and frame_1(X, Y) = T(X - U, Y - V) with the displacement given at the frame-1
    position, a = X - (width - 1) / 2, b = Y - (height - 1) / 2:
      bend:   U = 1.6 + kappa a b,       V = -0.7 - kappa a^2 / 2   (a beam's bending: uxy = kappa, vxx = -kappa)
      bulge:  U = 1.6 + kappa a^2 / 2,   V = -0.7 + kappa b^2 / 2   (uxx = vyy = kappa).
    gt_u, gt_v on frame 0's grid are the fixed point of (X, Y) = (x, y) + (U, V)(X, Y), 60 rounds -- a contraction by
    kappa * max(width, height) per round.  The names are in none of the other tuples of scene names."""
    if name not in SPECKLE_BENDINGS:
        raise ValueError("unknown speckle bending %r (one of %s)" % (name, ", ".join(SPECKLE_BENDINGS)))
    texture = Speckle(seed)
    kappa = float(kappa)
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0

    def displacement(x, y):
        a, b = np.asarray(x, np.float64) - cx, np.asarray(y, np.float64) - cy
        if name == "bend":
            return 1.6 + kappa * a * b, -0.7 - 0.5 * kappa * a * a
        return 1.6 + 0.5 * kappa * a * a, -0.7 + 0.5 * kappa * b * b

    def frame_1_at(x, y):
        du, dv = displacement(x, y)
        return texture(np.asarray(x, np.float64) - du, np.asarray(y, np.float64) - dv)

    def back_flow_at(x, y):
        du, dv = displacement(x, y)
        return -du, -dv

    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
    px, py = xs, ys
    for _ in range(60):
        du, dv = displacement(px, py)
        px, py = xs + du, ys + dv
    return Scene("speckle_" + name, texture(xs, ys).astype(np.float32), frame_1_at(xs, ys).astype(np.float32), (px - xs).astype(np.float32),
                 (py - ys).astype(np.float32), None, frame_1_at, frame_0_at=texture, back_flow_at=back_flow_at)


def make_speckle_deformation_sequence(name, steps=6, step_size=None, width=96, height=80, seed=0, translation=(0.0, 0.0)):
    """A loading sequence for the subset refinement over a sequence (flow2d_subset_refine_from_2d): the speckle pattern under k
    times the deformation `name` (one of SPECKLE_DEFORMATIONS) about the centre, k = 1 .. steps, every frame against the same
    frame 0.  step_size: the rotation's degrees per step (default 4), the stretch's e per step -- (1 + k e) x (1 - k e / 2),
    default 0.03 -- or the shear per step (default 0.04); translation: per step, on top.  Returns the list of the `steps` scenes
    of _affine_scene: scene k - 1 has frame_0, frame_1 = frame k and the exact displacement from frame 0 to frame k in gt_u, gt_v."""
    if steps < 1:
        raise ValueError("a deformation sequence has at least one step")
    if name not in SPECKLE_DEFORMATIONS:
        raise ValueError("unknown speckle deformation %r (one of %s)" % (name, ", ".join(SPECKLE_DEFORMATIONS)))
    texture = Speckle(seed)
    size = {"rotation": 4.0, "stretch": 0.03, "shear": 0.04}[name] if step_size is None else float(step_size)
    out = []
    for k in range(1, steps + 1):
        if name == "rotation":
            phi = np.radians(k * size)
            a = [[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]]
        elif name == "stretch":
            a = [[1.0 + k * size, 0.0], [0.0, 1.0 - k * size / 2.0]]
        else:
            a = [[1.0, k * size], [0.0, 1.0]]
        out.append(_affine_scene("speckle_%s_step_%d" % (name, k), width, height, texture, a, (k * translation[0], k * translation[1])))
    return out


class Scene:
    def __init__(self, name, frame_0, frame_1, gt_u, gt_v, occlusion, frame_1_at, frame_0_at=None, frame_at_time=None,
                 back_flow_at=None, occlusion_1=None):
        self.name = name
        self.frame_0, self.frame_1 = frame_0, frame_1
        self.gt_u, self.gt_v = gt_u, gt_v
        self.occlusion = occlusion
        self.frame_1_at = frame_1_at
        self.frame_0_at = frame_0_at
        self._frame_at_time = frame_at_time
        self.back_flow_at = back_flow_at
        self.occlusion_1 = occlusion_1
        ys, xs = np.mgrid[0:frame_0.shape[0], 0:frame_0.shape[1]].astype(np.float64)
        back_u, back_v = back_flow_at(xs, ys)
        self.gt_back_u, self.gt_back_v = back_u.astype(np.float32), back_v.astype(np.float32)

    def frame_at_time(self, t):
        """The exact frame at time t (float32, height x width): frame_0 at t = 0, frame_1 at t = 1."""
        return self._frame_at_time(float(t)).astype(np.float32)

    @property
    def shape(self):
        return self.frame_0.shape


def _affine_scene(name, width, height, texture, a, t):
    """W(x) = A (x - c) + c + t about the centre c; frame 1 = texture at W^-1, ground truth W(x) - x."""
    a = np.asarray(a, np.float64)
    t = np.asarray(t, np.float64)
    c = np.array([(width - 1) / 2.0, (height - 1) / 2.0])
    inv = np.linalg.inv(a)
    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)

    def frame_1_at(x, y):
        px, py = np.asarray(x, np.float64) - c[0] - t[0], np.asarray(y, np.float64) - c[1] - t[1]
        return texture(inv[0, 0] * px + inv[0, 1] * py + c[0], inv[1, 0] * px + inv[1, 1] * py + c[1])

    dx, dy = xs - c[0], ys - c[1]
    gt_u = (a[0, 0] - 1) * dx + a[0, 1] * dy + t[0]
    gt_v = a[1, 0] * dx + (a[1, 1] - 1) * dy + t[1]

    def frame_at_time(tau):
        # x -> x + tau * w(x) = c + (I + tau (A - I)) (x - c) + tau t: the texture at its inverse
        inv_t = np.linalg.inv(np.eye(2) + tau * (a - np.eye(2)))
        px, py = xs - c[0] - tau * t[0], ys - c[1] - tau * t[1]
        return texture(inv_t[0, 0] * px + inv_t[0, 1] * py + c[0], inv_t[1, 0] * px + inv_t[1, 1] * py + c[1])

    def back_flow_at(x, y):
        # y -> W^-1(y) = A^-1 (y - c - t) + c, so w_b(y) = W^-1(y) - y
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        px, py = x - c[0] - t[0], y - c[1] - t[1]
        return inv[0, 0] * px + inv[0, 1] * py + c[0] - x, inv[1, 0] * px + inv[1, 1] * py + c[1] - y

    return Scene(name, texture(xs, ys).astype(np.float32), frame_1_at(xs, ys).astype(np.float32), gt_u.astype(np.float32),
                 gt_v.astype(np.float32), None, frame_1_at, frame_0_at=texture, frame_at_time=frame_at_time,
                 back_flow_at=back_flow_at, occlusion_1=None)


def _two_layer_scene(width, height, background, square, t):
    """A side-n square at (x0, y0) in frame 0 moves by t (dyadic: x + t is exact in float32) over a static background."""
    n = max(4, min(width, height) // 4)
    x0, y0 = (width - n) // 2 - n // 4, (height - n) // 2
    tx, ty = t

    def in_square(x, y, sx, sy):
        return (x >= x0 + sx) & (x < x0 + n + sx) & (y >= y0 + sy) & (y < y0 + n + sy)

    def frame_1_at(x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return np.where(in_square(x, y, tx, ty), square(x - tx, y - ty), background(x, y))

    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
    moving = in_square(xs, ys, 0.0, 0.0)
    frame_0 = np.where(moving, square(xs, ys), background(xs, ys))
    gt_u = np.where(moving, tx, 0.0)
    gt_v = np.where(moving, ty, 0.0)
    covered = ~moving & in_square(xs, ys, tx, ty)
    leaving = moving & ((xs + tx < 0) | (xs + tx > width - 1) | (ys + ty < 0) | (ys + ty > height - 1))
    occlusion = (covered | leaving).astype(np.float32)

    def frame_0_at(x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return np.where(in_square(x, y, 0.0, 0.0), square(x, y), background(x, y))

    def frame_at_time(tau):
        sx, sy = tau * tx, tau * ty
        return np.where(in_square(xs, ys, sx, sy), square(xs - sx, ys - sy), background(xs, ys))

    # frame 1: the square's pixels move back by -t, the background stays; frame 1's occlusion: the background the square
    # uncovered, and square pixels whose backward vector leaves the frame
    def back_flow_at(x, y):
        shown = in_square(np.asarray(x, np.float64), np.asarray(y, np.float64), tx, ty)
        return np.where(shown, -tx, 0.0), np.where(shown, -ty, 0.0)

    shown = in_square(xs, ys, tx, ty)
    uncovered = ~shown & moving
    leaving_1 = shown & ((xs - tx < 0) | (xs - tx > width - 1) | (ys - ty < 0) | (ys - ty > height - 1))
    occlusion_1 = (uncovered | leaving_1).astype(np.float32)
    return Scene("two_layer", frame_0.astype(np.float32), frame_1_at(xs, ys).astype(np.float32), gt_u.astype(np.float32),
                 gt_v.astype(np.float32), occlusion, frame_1_at, frame_0_at=frame_0_at, frame_at_time=frame_at_time,
                 back_flow_at=back_flow_at, occlusion_1=occlusion_1)


def make_scene(name, width=256, height=256, seed=0):
    """The scene `name` (one of SCENES) at width x height; `seed` draws the textures."""
    rng = np.random.default_rng(seed)
    texture = Texture(rng)
    if name == "translation":
        return _affine_scene(name, width, height, texture, np.eye(2), (2.3, -1.4))
    if name == "rotation":
        phi = np.radians(3.0)
        return _affine_scene(name, width, height, texture, [[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]], (0, 0))
    if name == "zoom":
        return _affine_scene(name, width, height, texture, 1.03 * np.eye(2), (0, 0))
    if name == "affine":
        return _affine_scene(name, width, height, texture, [[1.02, 0.03], [-0.02, 0.985]], (1.25, -0.6))
    if name == "two_layer":
        square = Texture(rng, amplitude=(50.0, 35.0, 20.0), periods=(29.0, 13.1, 19.7))
        return _two_layer_scene(width, height, texture, square, (4.5, -2.25))
    raise ValueError("unknown scene %r (one of %s)" % (name, ", ".join(SCENES)))


class Sequence:
    def __init__(self, name, frame_count, width, height, frame_at, step, back_step, in_square=None, back_step_on=None):
        self.name = name
        # (x, y, k, on) -> position in frame k of the point at (x, y) in frame k + 1 (on: two_layer, the point's layer)
        self._back_step_on = back_step_on if back_step_on is not None else (lambda x, y, k, on: back_step(x, y, k))
        self.frame_count = frame_count
        self.width, self.height = width, height
        self.frame_at = frame_at
        self._step = step            # (x, y, k, on) -> position in frame k + 1 of the point at (x, y) in frame k (on: two_layer,
                                     # the point lies on the square)
        self._in_square = in_square  # two_layer: (x, y, k) -> the point lies on the square in frame k
        ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
        self.frames = np.stack([frame_at(k, xs, ys) for k in range(frame_count)]).astype(np.float32)
        fwd = [step(xs, ys, k, None if in_square is None else in_square(xs, ys, k)) for k in range(frame_count - 1)]
        bwd = [back_step(xs, ys, k) for k in range(frame_count - 1)]
        self.gt_u = np.stack([p[0] - xs for p in fwd]).astype(np.float32)
        self.gt_v = np.stack([p[1] - ys for p in fwd]).astype(np.float32)
        self.gt_back_u = np.stack([p[0] - xs for p in bwd]).astype(np.float32)
        self.gt_back_v = np.stack([p[1] - ys for p in bwd]).astype(np.float32)

    def _inside(self, x, y):
        return (x >= 0) & (x <= self.width - 1) & (y >= 0) & (y <= self.height - 1)

    def trajectory(self, x, y, k, start=0):
        """(x, y) in frame k (k >= start) of the point at (x, y) in frame `start`, in double."""
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        on = None if self._in_square is None else self._in_square(x, y, start)  # two_layer: the point's layer
        for j in range(start, k):
            x, y = self._step(x, y, j, on)
        return x, y

    def visible(self, x, y, k, start=0):
        """Whether the point at (x, y) in frame `start` is seen in frame k: inside the frame in every frame start .. k and, on
        two_layer, a background point not covered by the square in frame k."""
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        seen = self._inside(x, y)
        square = None if self._in_square is None else self._in_square(x, y, start)
        for j in range(start, k):
            x, y = self._step(x, y, j, square)
            seen = seen & self._inside(x, y)
        if square is not None:
            seen = seen & (square | ~self._in_square(x, y, k))
        return seen

    def trajectory_between(self, x, y, start, k):
        """trajectory for any pair of frames: (x, y) in frame k of the point at (x, y) in frame `start`, backwards (k < start)
        too -- the point keeps its layer on two_layer --, in double."""
        if k >= start:
            return self.trajectory(x, y, k, start)
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        on = None if self._in_square is None else self._in_square(x, y, start)
        for j in range(start - 1, k - 1, -1):
            x, y = self._back_step_on(x, y, j, on)
        return x, y

    def visible_between(self, x, y, start, k):
        """visible for any pair of frames: whether the point at (x, y) in frame `start` is seen in frame k, backwards too."""
        if k >= start:
            return self.visible(x, y, k, start)
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        seen = self._inside(x, y)
        square = None if self._in_square is None else self._in_square(x, y, start)
        for j in range(start - 1, k - 1, -1):
            x, y = self._back_step_on(x, y, j, square)
            seen = seen & self._inside(x, y)
        if square is not None:
            seen = seen & (square | ~self._in_square(x, y, k))
        return seen

    def flow_between(self, start, k):
        """The true flow of frame `start` to frame k on frame `start`'s grid, (u, v) float32 -- for neighbouring frames the
        values of gt_u / gt_v and gt_back_u / gt_back_v --, and the true visibility (bool): the pixel's content is seen in
        frame k."""
        ys, xs = np.mgrid[0:self.height, 0:self.width].astype(np.float64)
        px, py = self.trajectory_between(xs, ys, start, k)
        return (px - xs).astype(np.float32), (py - ys).astype(np.float32), self.visible_between(xs, ys, start, k)


def _affine_sequence(name, frame_count, width, height, texture, a, t):
    a = np.asarray(a, np.float64)
    t = np.asarray(t, np.float64)
    c = np.array([(width - 1) / 2.0, (height - 1) / 2.0])
    inv = np.linalg.inv(a)

    def back_step(x, y, k):  # W^-1, the operation order of _affine_scene's frame_1_at
        px, py = np.asarray(x, np.float64) - c[0] - t[0], np.asarray(y, np.float64) - c[1] - t[1]
        return inv[0, 0] * px + inv[0, 1] * py + c[0], inv[1, 0] * px + inv[1, 1] * py + c[1]

    def step(x, y, k, on=None):  # W
        dx, dy = np.asarray(x, np.float64) - c[0], np.asarray(y, np.float64) - c[1]
        return a[0, 0] * dx + a[0, 1] * dy + c[0] + t[0], a[1, 0] * dx + a[1, 1] * dy + c[1] + t[1]

    def frame_at(k, x, y):
        for _ in range(k):
            x, y = back_step(x, y, 0)
        return texture(x, y)

    return Sequence(name, frame_count, width, height, frame_at, step, back_step)


def _two_layer_sequence(frame_count, width, height, background, square, t):
    n = max(4, min(width, height) // 4)
    x0, y0 = (width - n) // 2 - n // 4, (height - n) // 2
    tx, ty = t

    def in_square(x, y, k):
        sx, sy = k * tx, k * ty
        return (x >= x0 + sx) & (x < x0 + n + sx) & (y >= y0 + sy) & (y < y0 + n + sy)

    def frame_at(k, x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return np.where(in_square(x, y, k), square(x - k * tx, y - k * ty), background(x, y))

    def step(x, y, k, on):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return np.where(on, x + tx, x), np.where(on, y + ty, y)

    def back_step(x, y, k):  # frame k + 1 -> frame k
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        on = in_square(x, y, k + 1)
        return np.where(on, x - tx, x), np.where(on, y - ty, y)

    def back_step_on(x, y, k, on):  # frame k + 1 -> frame k for a point of a known layer
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return np.where(on, x - tx, x), np.where(on, y - ty, y)

    return Sequence("two_layer", frame_count, width, height, frame_at, step, back_step, in_square, back_step_on)


def make_sequence(name, frame_count=10, width=256, height=256, seed=0):
    """The scene `name` (one of SCENES) carried on for frame_count (>= 2) frames; frames 0 and 1 are those of make_scene."""
    if frame_count < 2:
        raise ValueError("a sequence has at least two frames")
    rng = np.random.default_rng(seed)
    texture = Texture(rng)
    if name == "translation":
        return _affine_sequence(name, frame_count, width, height, texture, np.eye(2), (2.3, -1.4))
    if name == "rotation":
        phi = np.radians(3.0)
        return _affine_sequence(name, frame_count, width, height, texture,
                                [[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]], (0, 0))
    if name == "zoom":
        return _affine_sequence(name, frame_count, width, height, texture, 1.03 * np.eye(2), (0, 0))
    if name == "affine":
        return _affine_sequence(name, frame_count, width, height, texture, [[1.02, 0.03], [-0.02, 0.985]], (1.25, -0.6))
    if name == "two_layer":
        square = Texture(rng, amplitude=(50.0, 35.0, 20.0), periods=(29.0, 13.1, 19.7))
        return _two_layer_sequence(frame_count, width, height, texture, square, (4.5, -2.25))
    raise ValueError("unknown scene %r (one of %s)" % (name, ", ".join(SCENES)))


def make_speckle_sequence(motion, frame_count=4, width=96, height=80, seed=0):
    """The speckle scene `motion` (one of SPECKLE_MOTIONS) carried on for frame_count (>= 2) frames; frames 0 and 1 are those of
    make_speckle_scene.  With "large_translation" every pair moves by (11.25, -7.5): the case a warm-started sequence is for."""
    if frame_count < 2:
        raise ValueError("a sequence has at least two frames")
    texture = Speckle(seed)
    if motion == "translation":
        return _affine_sequence("speckle_translation", frame_count, width, height, texture, np.eye(2), (2.3, -1.4))
    if motion == "affine":
        return _affine_sequence("speckle_affine", frame_count, width, height, texture, [[1.02, 0.03], [-0.02, 0.985]], (1.25, -0.6))
    if motion == "large_translation":
        return _affine_sequence("speckle_large_translation", frame_count, width, height, texture, np.eye(2), (11.25, -7.5))
    raise ValueError("unknown speckle motion %r (one of %s)" % (motion, ", ".join(SPECKLE_MOTIONS)))
