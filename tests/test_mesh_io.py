"""rto_meshes_load / MeshSet.load: the basic OBJ reader and the drawlist npz (include/rto.h "meshes"; csrc/host/mesh_io.cpp).
The files are written here; what was loaded is read back from the set's records (MeshSet.download), which with an identity
transform hold the file's vertices as they are."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as M
import rt_octree_amd as R

E_IO, E_FORMAT = -5, -6
f32 = np.float32
DEFAULT = np.array([1.0, 0.5, 0.2], f32)


def _records(ms):
    prims, _ = ms.download()
    return prims[np.argsort(prims.view(np.uint32)[:, M.ID])]


def _load(path):
    return R.MeshSet.load(str(path), device=None)


def _rc(path):
    h = C.c_void_p(None)
    rc = R.lib().rto_meshes_load(str(path).encode(), -1, C.byref(h))
    assert (rc == 0) == bool(h.value)
    if rc == 0:
        R.lib().rto_meshes_free(h)
    return rc, R.lib().rto_last_error().decode()


def test_error_codes_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rto.h")).read()
    assert int(re.search(r"RTO_E_IO\s*=?\s*(-?\d+)", hdr).group(1)) == E_IO
    assert int(re.search(r"RTO_E_FORMAT\s*=?\s*(-?\d+)", hdr).group(1)) == E_FORMAT


OBJ = """# a square of two triangles, a pentagon that is dropped, and face forms
mtllib ignored.mtl
v 0 0 0 1 0 0
v 1 0 0 0 1 0
v 1 1 0   0 0 1
v 0 1 0 0.5 0.5 0.5
vt 0.5 0.5
vn 0 0 1
vn 0 0 1
vn 0 0 1
vn 0 0 1
v 0.5 0.5 1 1 1 0
vn 1 0 0
usemtl whatever
f 1 2 3
f 1/1 3/1 4/1
f 1/1/1 2/1/2 5/1/5
f -1//5 -2//4 -5//1
f 1 2 3 4 5
f 1 2
"""


def test_obj_forms_colours_normals_and_dropped_polygons(tmp_path):
    p = tmp_path / "a.obj"
    p.write_text(OBJ)
    ms = _load(p)
    assert (ms.triangles, ms.segments, ms.points) == (4, 0, 0)
    rec = _records(ms)
    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]], f32)
    col = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0.5], [1, 1, 0]], f32)
    nrm = np.array([[0, 0, 1]] * 4 + [[1, 0, 0]], f32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4], [4, 3, 0]])
    assert np.array_equal(rec[:, 0:9].reshape(-1, 3, 3), pos[faces])
    assert np.array_equal(rec[:, 9:18].reshape(-1, 3, 3), col[faces])
    assert np.array_equal(rec[:, 18:27].reshape(-1, 3, 3), nrm[faces])
    assert (rec.view(np.uint32)[:, M.KIND] == 3).all() and (rec.view(np.uint32)[:, M.UNLIT] == 0).all()


def test_obj_without_per_vertex_colours_and_normals_takes_the_defaults(tmp_path):
    p = tmp_path / "b.obj"
    p.write_text("v 0 0 0 1 0 0\nv 2 0 0\nv 0 2 0\nv 0 0 2\nvn 0 0 1\nf 1 2 3\nf 1 3 4\n")  # one colour of four, one normal of four
    rec = _records(_load(p))
    assert (rec[:, 9:18].reshape(-1, 3) == DEFAULT).all()
    m = R.Mesh(np.zeros((4, 9), f32), [[0, 1, 2], [0, 2, 3]])
    m.vert[:, :3] = [[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2]]
    m.vert[:, 3:6] = DEFAULT
    m.estimate = True
    assert np.array_equal(rec.view(np.uint32), M.bake([m]).view(np.uint32))  # estimated normals, as mesh_ref restates them
    assert np.allclose(rec[0, 21:24], [0, 0, 1])  # vertex 2 lies in the first triangle only


@pytest.mark.parametrize("text,what", [
    ("v 0 0 0\nv 1 0 0\nv 0 1", "three coordinates"),            # truncated inside a vertex line
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "out of range"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 -4\n", "out of range"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", "out of range"),
    ("v 0 0 zero\n", "no finite number"),
    ("v 0 0 nan\nv 1 0 0\nv 0 1 0\nf 1 2 3\n", "no finite number"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 x\n", "no face index"),
    ("\x00\x01\x02garbage\xff\n\x00", "NUL"),
    ("PK\x03\x04 this is no obj at all\n", "no vertices"),
    ("", "no vertices"),
])
def test_malformed_obj_is_refused_with_a_message(tmp_path, text, what):
    p = tmp_path / "bad.obj"
    p.write_bytes(text.encode("latin-1"))
    rc, msg = _rc(p)
    assert rc == E_FORMAT and what in msg and "bad.obj" in msg, msg


def test_missing_files_and_other_extensions(tmp_path):
    rc, msg = _rc(tmp_path / "nothing.obj")
    assert rc == E_IO and "cannot open" in msg
    rc, msg = _rc(tmp_path / "nothing.npz")
    assert rc == E_IO
    (tmp_path / "a.ply").write_text("ply\n")
    rc, msg = _rc(tmp_path / "a.ply")
    assert rc == E_FORMAT and "extension" in msg
    with pytest.raises(R.RtoError) as e:
        _load(tmp_path / "nothing.obj")
    assert e.value.code == E_IO


def _save(path, **kw):
    np.savez(str(path), **kw)
    return path


def test_drawlist_types_defaults_and_name_order(tmp_path):
    pts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 1]], np.float64)
    p = _save(tmp_path / "d.npz", **{
        "z_cube": "cube",
        "b_sphere": "Sphere", "b_sphere__rings": np.int64(5), "b_sphere__sectors": np.int32(6), "b_sphere__unlit": 1,
        "a_line": "line",
        "c_lines": "lines", "c_lines__points": pts.astype(np.float16), "c_lines__color": np.array([0.0, 1.0, 0.0]),
        "d_segs": "lines", "d_segs__points": pts.astype(f32), "d_segs__segs": np.array([[0, 2], [1, 3]], np.int16),
        "e_points": "points", "e_points__points": pts, "e_points__vert_color": np.eye(4, 3),
        "f_mesh": "mesh", "f_mesh__points": pts, "f_mesh__faces": np.array([[0, 1, 2], [0, 2, 3]]),
        "g_hidden": "cube", "g_hidden__visible": 0,
        "h_soup": "mesh", "h_soup__points": pts[:3], "h_soup__face_size": 3, "h_soup__translation": np.array([0.0, 0.0, 2.0]),
        "i_bad__too__deep": np.zeros(3),
    })
    ms = _load(p)
    rec = _records(ms)
    kinds = rec.view(np.uint32)[:, M.KIND]
    unlit = rec.view(np.uint32)[:, M.UNLIT]
    # name order: a_line, b_sphere (4 * 6 * 2 = 48), c_lines (3), d_segs (2), e_points (4), f_mesh (2), h_soup (1), z_cube (12)
    counts = [1, 48, 3, 2, 4, 2, 1, 12]
    assert list(kinds) == [2] + [3] * 48 + [2] * 3 + [2] * 2 + [1] * 4 + [3] * 2 + [3] + [3] * 12
    at = np.concatenate([[0], np.cumsum(counts)])
    line, sphere, lines, segs, points, mesh, soup, cube = (rec[at[i]:at[i + 1]] for i in range(8))
    assert np.array_equal(line[0, 0:6], [0, 0, 0, 0, 0, 1]) and (line[0, 9:15].reshape(2, 3) == DEFAULT).all()  # a = 0, b = +z
    assert (unlit[at[1]:at[2]] == 1).all() and (unlit[at[5]:at[6]] == 0).all() and (unlit[at[7]:] == 0).all()  # unlit defaults to 0
    assert np.array_equal(lines[:, 0:6].reshape(3, 2, 3), pts.astype(f32)[[[0, 1], [1, 2], [2, 3]]])
    assert (lines[:, 9:15].reshape(-1, 3) == np.array([0, 1, 0], f32)).all()
    assert np.array_equal(segs[:, 0:6].reshape(2, 2, 3), pts.astype(f32)[[[0, 2], [1, 3]]])
    assert np.array_equal(points[:, 0:3], pts.astype(f32)) and np.array_equal(points[:, 9:12], np.eye(4, 3, dtype=f32))
    assert np.array_equal(mesh[:, 0:9].reshape(2, 3, 3), pts.astype(f32)[[[0, 1, 2], [0, 2, 3]]])
    assert np.allclose(mesh[0, 21:24], [0, 0, 1])  # estimated: vertex 1 lies in the flat first triangle only
    assert np.array_equal(soup[0, 0:9].reshape(3, 3), pts[:3].astype(f32) + np.array([0, 0, 2], f32))
    # the presets equal the Python generators (closed forms below)
    sp = R.Mesh.Sphere(5, 6)
    sp.unlit = True
    assert np.array_equal(sphere.view(np.uint32)[:, :27], M.bake([sp]).view(np.uint32)[:, :27])
    assert np.array_equal(cube.view(np.uint32)[:, :27], M.bake([R.Mesh.Cube()]).view(np.uint32)[:, :27])


def test_presets_equal_their_closed_forms(tmp_path):
    sp = R.Mesh.Sphere(15, 30)
    assert sp.vert.shape == (450, 9) and sp.faces.shape == (840, 3) and sp.faces.max() == 449
    assert np.allclose(np.linalg.norm(sp.vert[:, :3].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.array_equal(sp.vert[:, :3], sp.vert[:, 6:])  # the normal is the position
    assert np.allclose(sp.vert[0, :3], [0, 0, -1], atol=1e-7) and np.allclose(sp.vert[-1, :3], [0, 0, 1], atol=1e-7)
    # every edge between two rings is shared by exactly two triangles: the surface is closed around the axis
    e = np.sort(np.concatenate([sp.faces[:, [0, 1]], sp.faces[:, [1, 2]], sp.faces[:, [2, 0]]]).astype(np.int64), axis=1)
    ring = e[:, 0] // 30 != e[:, 1] // 30
    _, cnt = np.unique(e[ring], axis=0, return_counts=True)
    assert (cnt == 2).all()
    cube = R.Mesh.Cube((0.1, 0.2, 0.3))
    v = cube.vert.reshape(6, 6, 9)
    assert (np.abs(v[..., :3]) == 0.5).all() and (v[..., 3:6] == np.array([0.1, 0.2, 0.3], f32)).all()
    for f, (axis, sign) in enumerate(((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1))):
        n = np.zeros(3, f32)
        n[axis] = sign
        assert (v[f, :, 6:] == n).all() and (v[f, :, axis] == 0.5 * sign).all()
        assert len({tuple(p) for p in v[f, :, :3]}) == 4  # two triangles over the face's four corners
        for tri in v[f].reshape(2, 3, 9):
            c = np.cross(tri[1, :3] - tri[0, :3], tri[2, :3] - tri[0, :3])
            assert abs(c[axis]) == 1.0  # each half the unit face
    fr = R.Mesh.CameraFrustum(100.0, 80.0, 60.0, -0.5)
    want = np.array([[0, 0, 0], [0.2, 0.15, -0.5], [0.2, -0.15, -0.5], [-0.2, -0.15, -0.5], [-0.2, 0.15, -0.5]], f32)
    assert np.allclose(fr.vert[:, :3], want, atol=1e-7) and fr.face_size == 2 and fr.unlit and len(fr.faces) == 8
    assert sorted(map(tuple, np.sort(fr.faces, 1))) == [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 4), (2, 3), (3, 4)]
    lat = R.Mesh.Lattice(4)
    assert lat.vert.shape == (64, 9) and lat.face_size == 1 and np.allclose(lat.vert[:, :3].mean(0), 0.5)
    # the drawlist's frusta: defaults (1111, 800, 800, -0.3), r / t copies, connect
    r = np.array([[0, 0, 0], [0, 0, np.pi / 2], [0.3, -0.2, 0.1]])
    t = np.array([[0, 0, 0], [1, 2, 3], [-1, 0.5, 0]])
    p = _save(tmp_path / "f.npz", cams="camerafrustum", cams__r=r, cams__t=t, cams__connect=1, cams__color=np.array([0.0, 0.0, 1.0]))
    ms = _load(p)
    assert (ms.triangles, ms.segments, ms.points) == (0, 3 * 8 + 2, 0)
    rec = _records(ms)
    base = R.Mesh.CameraFrustum(1111.0, 800.0, 800.0, -0.3).vert[:, :3].astype(np.float64)
    for k in range(3):
        m = R.Mesh.Points(np.zeros((1, 3))).placed(r[k], (0, 0, 0), 1.0)
        want = (base @ M.model_matrix(m).T + t[k]).astype(f32)
        got = rec[8 * k:8 * k + 8, 0:6].reshape(8, 2, 3)
        assert np.allclose(got, want[fr.faces.astype(np.int64)], atol=1e-6), k
    assert np.allclose(rec[24:, 0:6].reshape(2, 2, 3), np.stack([t[:2], t[1:]]).astype(f32), atol=1e-6)
    assert (rec[:, 9:15].reshape(-1, 3) == np.array([0, 0, 1], f32)).all()


def test_several_files_are_concatenated_in_order(tmp_path):
    a = tmp_path / "a.obj"
    a.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    b = _save(tmp_path / "b.npz", pts="points", pts__points=np.zeros((2, 3)))
    ms = R.MeshSet.load([str(a), str(b), str(a)], device=None)
    assert list(_records(ms).view(np.uint32)[:, M.KIND]) == [3, 1, 1, 3]


def test_malformed_drawlists_are_refused_with_a_message(tmp_path):
    pts = np.zeros((4, 3))
    cases = {
        "unsupported type": dict(a="teapot"),
        "out of range": dict(a="mesh", a__points=pts, a__faces=np.array([[0, 1, 4]])),
        "index is out of range": dict(a="lines", a__points=pts, a__segs=np.array([[0, -1]])),
        "divisible by 3": dict(a="points", a__points=np.zeros(7)),
        "multiple of the face size": dict(a="mesh", a__points=pts, a__faces=np.array([0, 1, 2, 3])),
        "face_size must be": dict(a="mesh", a__points=pts, a__face_size=4),
        "vert_color has the wrong size": dict(a="points", a__points=pts, a__vert_color=np.zeros((3, 3))),
        "not a float array": dict(a="points", a__points=np.array(["x", "y", "z"])),
        "no string": dict(a=np.zeros(3)),
        "shape (3,)": dict(a="cube", a__color=np.zeros(4)),
        "rings or sectors": dict(a="sphere", a__rings=1),
        "non-finite": dict(a="points", a__points=np.array([[0.0, np.nan, 0.0]])),
        "r and t differ": dict(a="camerafrustum", a__r=np.zeros((2, 3)), a__t=np.zeros((3, 3))),
    }
    for what, kw in cases.items():
        rc, msg = _rc(_save(tmp_path / "bad.npz", **kw))
        assert rc == E_FORMAT and what in msg, (what, msg)
    good = _save(tmp_path / "good.npz", a="mesh", a__points=pts, a__faces=np.array([[0, 1, 2]]), b="sphere")
    raw = good.read_bytes()
    assert _rc(good)[0] == 0
    for cut in (len(raw) - 10, len(raw) // 2, 40, 3):
        (tmp_path / "cut.npz").write_bytes(raw[:cut])
        rc, msg = _rc(tmp_path / "cut.npz")
        assert rc == E_FORMAT and msg, cut
    rng = np.random.default_rng(1)
    (tmp_path / "junk.npz").write_bytes(rng.integers(0, 256, 3000, dtype=np.uint8).tobytes())
    assert _rc(tmp_path / "junk.npz")[0] == E_FORMAT


def test_python_descriptions_build_the_set_the_c_loaders_build(tmp_path):
    """Mesh.load_basic_obj / Mesh.open_drawlist restate the two readers in numpy: MeshSet of their descriptions holds the records
    of MeshSet.load of the same files, bit for bit"""
    a = tmp_path / "a.obj"
    a.write_text(OBJ)
    b = tmp_path / "b.obj"
    b.write_text("v 0 0 0 1 0 0\nv 2 0 0\nv 0 2 0\nv 0 0 2\nvn 0 0 1\nf 1 2 3\nf 1 3 4\n")
    pts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 1]], np.float64)
    rng = np.random.default_rng(4)
    d = _save(tmp_path / "d.npz", **{
        "z_cube": "cube", "z_cube__rotation": np.array([0.3, 0.2, -0.5]), "z_cube__scale": 0.7,
        "b_sphere": "sphere", "b_sphere__rings": 5, "b_sphere__sectors": 6, "b_sphere__unlit": 1, "b_sphere__translation": np.array([0.1, 0.2, 0.3]),
        "a_line": "line", "a_line__b": np.array([1.0, 2.0, 3.0]),
        "c_lines": "lines", "c_lines__points": pts.astype(np.float16), "c_lines__color": np.array([0.0, 1.0, 0.0]),
        "d_segs": "lines", "d_segs__points": pts.astype(f32), "d_segs__segs": np.array([[0, 2], [1, 3]], np.int16),
        "e_points": "points", "e_points__points": pts, "e_points__vert_color": np.eye(4, 3),
        "f_mesh": "mesh", "f_mesh__points": pts, "f_mesh__faces": np.array([[0, 1, 2], [0, 2, 3]]),
        "g_hidden": "cube", "g_hidden__visible": 0,
        "h_soup": "mesh", "h_soup__points": pts[:3],
        "k_cams": "camerafrustum", "k_cams__r": rng.uniform(-1, 1, (4, 3)), "k_cams__t": rng.uniform(-1, 1, (4, 3)), "k_cams__connect": 1,
        "l_one": "camerafrustum", "l_one__focal_length": 50.0, "l_one__image_width": 64.0, "l_one__z": -1.0,
    })
    for path in (a, b):
        m = R.Mesh.load_basic_obj(str(path))
        assert np.array_equal(_records(R.MeshSet([m], device=None)).view(np.uint32), _records(_load(path)).view(np.uint32)), path
    meshes = R.Mesh.open_drawlist(str(d))
    assert [m.name for m in meshes] == sorted(m.name for m in meshes) and len(meshes) == 11
    assert [m.name for m in meshes if not m.visible] == ["g_hidden"]
    assert np.array_equal(_records(R.MeshSet(meshes, device=None)).view(np.uint32), _records(_load(d)).view(np.uint32))
    with pytest.raises(R.RtoError) as e:
        R.Mesh.load_basic_obj(str(_write(tmp_path / "bad.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")))
    assert e.value.code == E_FORMAT
    with pytest.raises(R.RtoError) as e:
        R.Mesh.open_drawlist(str(_save(tmp_path / "bad.npz", a="teapot")))
    assert e.value.code == E_FORMAT


def _write(path, text):
    path.write_text(text)
    return path
