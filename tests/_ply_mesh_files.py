"""PLY mesh files for the reader's tests (tests/test_mesh_host_cpu.py, tests/test_ply_mesh_cpu.py, tests/test_gpu_mesh_host.py)."""
import struct

import numpy as np

_FMT = {"uchar": "<B", "char": "<b", "ushort": "<H", "short": "<h", "uint": "<I", "int": "<i", "float": "<f", "double": "<d"}


def write_ply_mesh(path, vertices, faces, binary=True, count_type="uchar", index_type="int", list_name="vertex_indices",
                   vertex_type="double", face_extra=False, edges=0):
    """faces: a list of index tuples (any length); face_extra adds a `uchar flag` property BEFORE and a `float quality` AFTER the list;
    edges > 0 appends an `edge` element of that many rows after the faces."""
    hdr = ["ply", "format " + ("binary_little_endian" if binary else "ascii") + " 1.0", "comment written by a test",
           f"element vertex {len(vertices)}"] + [f"property {vertex_type} {a}" for a in "xyz"] + [f"element face {len(faces)}"]
    if face_extra:
        hdr.append("property uchar flag")
    hdr.append(f"property list {count_type} {index_type} {list_name}")
    if face_extra:
        hdr.append("property float quality")
    if edges:
        hdr += [f"element edge {edges}", "property int vertex1", "property int vertex2"]
    hdr.append("end_header")
    body = bytearray()
    text = []
    for v in np.asarray(vertices, np.float64):
        if binary:
            body += b"".join(struct.pack(_FMT[vertex_type], x) for x in v)
        else:
            text.append(" ".join(repr(float(x)) for x in v))
    for k, fc in enumerate(faces):
        if binary:
            if face_extra:
                body += struct.pack("<B", k % 7)
            body += struct.pack(_FMT[count_type], len(fc)) + b"".join(struct.pack(_FMT[index_type], int(i)) for i in fc)
            if face_extra:
                body += struct.pack("<f", 0.5 * k)
        else:
            text.append(" ".join(([str(k % 7)] if face_extra else []) + [str(len(fc))] + [str(int(i)) for i in fc]
                                 + ([repr(0.5 * k)] if face_extra else [])))
    for k in range(edges):
        if binary:
            body += struct.pack("<ii", k, k + 1)
        else:
            text.append(f"{k} {k + 1}")
    with open(path, "wb") as f:
        f.write(("\n".join(hdr) + "\n").encode())
        f.write(bytes(body) if binary else ("\n".join(text) + "\n").encode())
    return path


def fan(faces):
    """the triangles the reader makes of the polygons: (0, k, k + 1)"""
    return np.array([(fc[0], fc[k], fc[k + 1]) for fc in faces for k in range(1, len(fc) - 1)], np.int32).reshape(-1, 3)
