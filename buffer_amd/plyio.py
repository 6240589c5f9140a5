"""File formats the 3DMatch-layout test sets share (host only): .ply point clouds and the gt.log pose list."""
import os

import numpy as np

_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
              'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
              'double': 'f8', 'float64': 'f8'}


def read_ply(path, drop_non_finite=False):
    """Vertex positions of a .ply point cloud (ascii, binary_little_endian or binary_big_endian) -> f32[n,3].
    (open3d.io.read_point_cloud in utils/tools.py:6-7; only x, y, z are used by the reference.)
    drop_non_finite: leave out every row with a NaN or inf coordinate, as open3d's read_point_cloud does by default
    (remove_nan_points / remove_infinite_points); off by default, so a row reaches the caller as stored."""
    with open(path, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise ValueError(f'{path}: not a PLY file')
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f'{path}: truncated PLY header')
            tok = line.decode('ascii', 'replace').split()
            if not tok or tok[0] == 'comment' or tok[0] == 'obj_info':
                continue
            if tok[0] == 'format':
                fmt = tok[1]
            elif tok[0] == 'element':
                elements.append([tok[1], int(tok[2]), []])
            elif tok[0] == 'property':
                if tok[1] == 'list':
                    elements[-1][2].append((tok[4], 'list', tok[2], tok[3]))
                else:
                    elements[-1][2].append((tok[2], tok[1]))
            elif tok[0] == 'end_header':
                break
        if not elements or elements[0][0] != 'vertex':
            raise ValueError(f'{path}: the first PLY element is not "vertex"')
        _, n, props = elements[0]
        if any(p[1] == 'list' for p in props):
            raise ValueError(f'{path}: list property in the vertex element')
        names = [p[0] for p in props]
        if not all(k in names for k in 'xyz'):
            raise ValueError(f'{path}: vertex element has no x/y/z')
        if fmt == 'ascii':
            rows = np.loadtxt(f, dtype=np.float64, max_rows=n, ndmin=2) if n else np.zeros((0, len(props)))
            cols = [rows[:, names.index(k)] for k in 'xyz']
        elif fmt in ('binary_little_endian', 'binary_big_endian'):
            end = '<' if fmt == 'binary_little_endian' else '>'
            dt = np.dtype([(p[0], end + _PLY_TYPES[p[1]]) for p in props])
            rows = np.frombuffer(f.read(dt.itemsize * n), dtype=dt, count=n)
            cols = [rows[k] for k in 'xyz']
        else:
            raise ValueError(f'{path}: unknown PLY format {fmt}')
    pts = np.stack(cols, axis=1).astype(np.float32)
    if drop_non_finite:
        pts = np.ascontiguousarray(pts[np.isfinite(pts).all(axis=1)])
    return pts


def write_ply(path, pts):
    """f32[n,3] -> binary_little_endian PLY (tools and tests)."""
    pts = np.ascontiguousarray(pts, dtype='<f4')
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        f.write(b'ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n'
                b'property float z\nend_header\n' % pts.shape[0])
        f.write(pts.tobytes())


def load_gt_log(gtpath):
    """utils/tools.py:47-62: gt.log -> {'i_j': f64[4,4]} in file order."""
    with open(os.path.join(gtpath, 'gt.log')) as f:
        content = f.readlines()
    result = {}
    for i in range(0, len(content) - 4, 5):
        head = content[i].replace("\n", "").split("\t")[0:3]
        trans = np.array([[float(x) for x in content[i + r].replace("\n", "").split("\t")[0:4]] for r in range(1, 5)])
        result[f'{int(head[0])}_{int(head[1])}'] = trans
    return result
