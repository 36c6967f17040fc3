"""quat_standin.Quaternion plus the three read-outs that the reference's motion_processing takes from a box's orientation
(datasets/sampler.py:148-155): `.radians`, `.degrees` and `.axis` (TEST ONLY, for tests/golden/make_golden_motion_batches.py).
They have pyquaternion's documented meaning: the rotation angle 2 atan2(|v|, w) of the normalised quaternion wrapped into
(-pi, pi], and the unit rotation axis v / |v|, the zero vector for the identity (|v| below 1e-17).  Every operation of the
base class that returns a quaternion returns this class, so that a box's orientation keeps the read-outs through the
reference's products and inverses."""
import numpy as np

import quat_standin


class Quaternion(quat_standin.Quaternion):
    @property
    def inverse(self):
        return Quaternion(super().inverse)

    def __mul__(self, o):
        return Quaternion(super().__mul__(o))

    @property
    def radians(self):
        q = self.q / np.linalg.norm(self.q)
        theta = 2.0 * np.arctan2(np.linalg.norm(q[1:]), q[0])
        wrapped = ((theta + np.pi) % (2 * np.pi)) - np.pi
        return np.pi if wrapped == -np.pi else wrapped

    angle = radians

    @property
    def degrees(self):
        return self.radians * 180.0 / np.pi

    @property
    def axis(self):
        q = self.q / np.linalg.norm(self.q)
        n = np.linalg.norm(q[1:])
        return np.zeros(3) if n < 1e-17 else q[1:] / n
