"""A small unit-quaternion class for the fixture generators (TEST ONLY): pyquaternion is not installed where the fixtures
are made, and the reference's datasets/data_classes.py + datasets/points_utils.py need only this much of it --
Quaternion(matrix=...), Quaternion(axis=..., degrees= | radians=...), `.inverse`, `*`, `.rotation_matrix`, `.elements`.
Written from the textbook formulas (Hamilton product, Shepperd's matrix-to-quaternion), in float64."""
import numpy as np


class Quaternion:
    def __init__(self, *args, matrix=None, axis=None, degrees=None, radians=None):
        if matrix is not None:
            self.q = self._from_matrix(np.asarray(matrix, np.float64))
        elif axis is not None:
            angle = float(radians) if radians is not None else float(degrees) * np.pi / 180.0
            a = np.asarray(axis, np.float64)
            a = a / np.linalg.norm(a)
            self.q = np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])
        elif len(args) == 1:
            self.q = np.asarray(args[0].q if isinstance(args[0], Quaternion) else args[0], np.float64).reshape(4).copy()
        elif len(args) == 4:
            self.q = np.asarray(args, np.float64)
        else:
            self.q = np.array([1.0, 0.0, 0.0, 0.0])

    @staticmethod
    def _from_matrix(m):
        t = np.trace(m[:3, :3])
        if t > 0:
            s = 2 * np.sqrt(1 + t)
            q = [s / 4, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
        else:
            i = int(np.argmax([m[0, 0], m[1, 1], m[2, 2]]))
            j, k = (i + 1) % 3, (i + 2) % 3
            s = 2 * np.sqrt(1 + m[i, i] - m[j, j] - m[k, k])
            q = [0.0, 0.0, 0.0, 0.0]
            q[0] = (m[k, j] - m[j, k]) / s
            q[1 + i] = s / 4
            q[1 + j] = (m[j, i] + m[i, j]) / s
            q[1 + k] = (m[k, i] + m[i, k]) / s
        q = np.asarray(q, np.float64)
        return q / np.linalg.norm(q)

    @property
    def elements(self):
        return self.q

    @property
    def inverse(self):
        n = float(self.q @ self.q)
        return Quaternion(np.array([self.q[0], -self.q[1], -self.q[2], -self.q[3]]) / n)

    def __mul__(self, o):
        a, b = self.q, o.q
        return Quaternion(np.array([
            a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]))

    @property
    def rotation_matrix(self):
        w, x, y, z = self.q / np.linalg.norm(self.q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
