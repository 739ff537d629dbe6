"""Meshes for the layered render path: descriptions (Mesh), mesh sets on the device (MeshSet) and the passes that draw them
(draw_mesh_layers, trace_mesh_rays) over the C ABI of include/rto.h "meshes".

Mesh mirrors the reference's volrend::Mesh (renderer/include/volrend/mesh.hpp, src/mesh.cpp): vert [n, 9] float32 (position, rgb,
normal), faces [m, face_size] uint32 or None, face_size 3 / 2 / 1, unlit, and the model transform (rotation axis-angle,
translation, scale) that MeshSet bakes into world space.  The preset generators are written from the shapes' definitions."""
import ctypes as C

import numpy as np

from ._lib import CMeshDesc, CMeshesInfo, CMeshParams, CMeshRays, LayerParams, RtoError, check, lib

MESH_MERGE = 1  # RTO_MESH_MERGE (draw_mesh_layers(merge=True))
DEFAULT_COLOR = (1.0, 0.5, 0.2)
f32 = np.float32


def _rotation_matrix(r):
    """axis-angle -> 3x3 float64, |r| < 1e-3 the identity (Mesh::apply_transform; host/mesh_io.cpp rotation_matrix)"""
    r = np.asarray(r, f32).astype(np.float64)
    ang = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    M = np.eye(3)
    if not ang < 1e-3:
        a = r / ang
        c, s = np.cos(ang), np.sin(ang)
        k = 1.0 - c
        X = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        for i in range(3):
            for j in range(3):
                M[i, j] = ((c if i == j else 0.0) + k * (a[i] * a[j])) + s * X[i, j]
    return M


class Mesh:
    def __init__(self, vert, faces=None, face_size=3, unlit=False, name="Mesh"):
        self.vert = np.ascontiguousarray(vert, f32).reshape(-1, 9)
        self.faces = None if faces is None else np.ascontiguousarray(faces, np.uint32).reshape(-1, face_size)
        self.face_size = int(face_size)
        self.unlit = bool(unlit)
        self.name = name
        self.rotation = np.zeros(3, f32)
        self.translation = np.zeros(3, f32)
        self.scale = 1.0
        self.visible = True
        self.estimate = False  # rto_mesh_desc.estimate_normals

    def placed(self, rotation=None, translation=None, scale=None):
        """the model transform of Mesh::draw, set in place; returns self"""
        if rotation is not None:
            self.rotation = np.asarray(rotation, f32).reshape(3)
        if translation is not None:
            self.translation = np.asarray(translation, f32).reshape(3)
        if scale is not None:
            self.scale = float(scale)
        return self

    @property
    def n_faces(self):
        return len(self.faces) if self.faces is not None else len(self.vert) // self.face_size

    @staticmethod
    def _from_points(points, color, normal, faces, face_size, unlit, name):
        p = np.asarray(points, f32).reshape(-1, 3)
        v = np.empty((len(p), 9), f32)
        v[:, :3] = p
        v[:, 3:6] = np.asarray(color, f32)
        v[:, 6:] = np.asarray(normal, f32)
        return Mesh(v, faces, face_size, unlit, name)

    @staticmethod
    def Cube(color=DEFAULT_COLOR):
        """the cube [-0.5, 0.5]^3 as 12 triangles of 36 unshared vertices, generated from its six face normals -z, +z, -y, +y,
        -x, +x (the reference's face order); every vertex carries its face's normal"""
        verts = []
        for axis, sign in ((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1)):
            a, b = [i for i in range(3) if i != axis]
            n = np.zeros(3, f32)
            n[axis] = sign
            for ca, cb in ((-0.5, -0.5), (0.5, 0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, -0.5), (-0.5, 0.5)):
                p = np.zeros(3, f32)
                p[axis], p[a], p[b] = 0.5 * sign, ca, cb
                verts.append(np.concatenate([p, np.asarray(color, f32), n]))
        return Mesh(np.stack(verts), None, 3, False, "Cube")

    @staticmethod
    def Sphere(rings=15, sectors=30, color=DEFAULT_COLOR):
        """the unit UV sphere: vertex (r, s) at latitude -pi/2 + r pi / (rings - 1) and longitude 2 pi s / sectors, its normal its
        position; two triangles per quad between neighbouring rings: (rings - 1) * sectors * 2 faces"""
        r = np.arange(rings, dtype=np.float64)[:, None] * (np.pi / (rings - 1))
        s = np.arange(sectors, dtype=np.float64)[None, :] * (2.0 * np.pi / sectors)
        z = np.broadcast_to(np.sin(r - 0.5 * np.pi), (rings, sectors))
        x, y = np.cos(s) * np.sin(r), np.sin(s) * np.sin(r)
        p = np.stack([x, y, z], -1).reshape(-1, 3).astype(f32)
        rr, ss = np.meshgrid(np.arange(rings - 1), np.arange(sectors), indexing="ij")
        ns = (ss + 1) % sectors
        quad = np.stack([rr * sectors + ns, rr * sectors + ss, (rr + 1) * sectors + ss,
                         (rr + 1) * sectors + ss, (rr + 1) * sectors + ns, rr * sectors + ns], -1)
        m = Mesh._from_points(p, color, p, quad.reshape(-1, 3), 3, False, "Sphere")
        return m

    @staticmethod
    def Lattice(reso=8, color=DEFAULT_COLOR):
        """reso^3 points at the cell centres of the unit cube"""
        c = (np.arange(reso, dtype=f32) + f32(0.5)) / f32(reso)
        p = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
        return Mesh._from_points(p, color, (1, 0, 0), None, 1, True, "Lattice")

    @staticmethod
    def CameraFrustum(focal_length, image_width, image_height, z=-0.3, color=DEFAULT_COLOR):
        """the apex at the origin and the image rectangle at depth z, as 8 lines: four from the apex, four around the rectangle"""
        hw, hh = f32(0.5) * f32(image_width), f32(0.5) * f32(image_height)
        inv, z = f32(1) / f32(focal_length), f32(z)
        corners = [(-hw, -hh), (-hw, hh), (hw, hh), (hw, -hh)]
        p = [(0, 0, 0)] + [(z * cx * inv, z * cy * inv, z) for cx, cy in corners]
        faces = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4), (4, 1)]
        return Mesh._from_points(p, color, (0, 0, 1), faces, 2, True, "CameraFrustum")

    @staticmethod
    def Line(a, b, color=DEFAULT_COLOR):
        return Mesh._from_points([a, b], color, (0, 0, 1), [(0, 1)], 2, True, "Line")

    @staticmethod
    def Lines(points, color=DEFAULT_COLOR, segs=None):
        """a polyline through `points` [n, 3], or the segments `segs` [m, 2] between them"""
        p = np.asarray(points, f32).reshape(-1, 3)
        if segs is None:
            segs = np.stack([np.arange(len(p) - 1), np.arange(1, len(p))], 1)
        return Mesh._from_points(p, color, (0, 0, 1), segs, 2, True, "Lines")

    @staticmethod
    def Points(points, color=DEFAULT_COLOR):
        return Mesh._from_points(points, color, (0, 0, 1), None, 1, True, "Points")

    @staticmethod
    def load_basic_obj(path):
        """Mesh::load_basic_obj as rto_meshes_load reads an .obj (csrc/host/mesh_io.cpp), restated for a numpy description:
        `v x y z [r g b]`, `vn`, `f` with a, a/b, a/b/c, a//c and negative indices; polygons that are no triangles are dropped;
        colours / normals only when there is one per vertex, else (1, 0.5, 0.2) and estimated normals (Mesh.estimate)"""
        pos, col, nrm, faces, n_col = [], [], [], [], 0
        with open(path, "rb") as f:
            data = f.read()
        if b"\0" in data:
            raise RtoError(-6, "load_basic_obj: %s holds a NUL byte: not a text file" % path)
        for no, line in enumerate(data.decode("latin-1").split("\n"), 1):
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            try:
                if tok[0] == "v":
                    v = [float(np.float32(t)) for t in tok[1:8]]
                    if len(v) < 3 or not np.isfinite(v).all():
                        raise ValueError("a vertex needs three finite coordinates")
                    pos.append(v[:3])
                    col.append(v[3:6] if len(v) >= 6 else list(DEFAULT_COLOR))
                    n_col += len(v) >= 6
                elif tok[0] == "vn":
                    v = [float(np.float32(t)) for t in tok[1:4]]
                    if len(v) < 3 or not np.isfinite(v).all():
                        raise ValueError("a normal needs three finite coordinates")
                    nrm.append(v)
                elif tok[0] == "f":
                    ix = []
                    for t in tok[1:]:
                        a = int(t.split("/", 1)[0])
                        k = a - 1 if a > 0 else a + len(pos)
                        if a == 0 or not 0 <= k < len(pos):
                            raise ValueError("face index %d is out of range" % a)
                        ix.append(k)
                    if len(ix) == 3:
                        faces.append(ix)
            except ValueError as e:
                raise RtoError(-6, "load_basic_obj: %s line %d: %s" % (path, no, e))
        if not pos:
            raise RtoError(-6, "load_basic_obj: %s: no vertices" % path)
        v = np.zeros((len(pos), 9), f32)
        v[:, :3] = np.asarray(pos, f32)
        v[:, 3:6] = np.asarray(col, f32) if n_col == len(pos) else np.asarray(DEFAULT_COLOR, f32)
        if len(nrm) == len(pos):
            v[:, 6:] = np.asarray(nrm, f32)
        if not faces:
            v = v[:0]
        m = Mesh(v, np.asarray(faces, np.uint32).reshape(-1, 3), 3, False, str(path))
        m.estimate = len(nrm) != len(pos)
        return m

    @staticmethod
    def open_drawlist(path, default_visible=True):
        """Mesh::open_drawlist as rto_meshes_load reads a drawlist .npz, restated for numpy descriptions: the meshes in the order
        of their names, invisible ones included (MeshSet leaves them out)"""
        z = np.load(path, allow_pickle=False)
        parsed = {}
        for key in z.files:
            name, sep, field = key.partition("__")
            if not sep:
                parsed.setdefault(name, ["", {}])[0] = str(z[key]).lower()
            elif name and field and "__" not in field:
                parsed.setdefault(name, ["", {}])[1][field] = z[key]
        out = []
        for name in sorted(parsed):
            kind, f = parsed[name]

            def vec3(k, d):
                return np.asarray(f[k], f32).reshape(3) if k in f else np.asarray(d, f32)

            def pts(k="points"):
                return np.asarray(f[k], f32).reshape(-1, 3) if k in f else np.zeros((0, 3), f32)

            color = vec3("color", DEFAULT_COLOR)
            if kind == "cube":
                m = Mesh.Cube(color)
            elif kind == "sphere":
                m = Mesh.Sphere(int(f.get("rings", 15)), int(f.get("sectors", 30)), color)
            elif kind == "line":
                m = Mesh.Line(vec3("a", (0, 0, 0)), vec3("b", (0, 0, 1)), color)
            elif kind == "camerafrustum":
                m = Mesh.CameraFrustum(f32(f.get("focal_length", 1111.0)), f32(f.get("image_width", 800.0)),
                                       f32(f.get("image_height", 800.0)), f32(f.get("z", -0.3)), color)
                if "t" in f:
                    t, r = pts("t"), pts("r")
                    if t.shape != r.shape:
                        raise RtoError(-6, "open_drawlist: mesh '%s': r and t differ in size" % name)
                    base, verts, faces = m.vert[:, :3].astype(np.float64), [], []
                    for k in range(len(t)):
                        M = _rotation_matrix(r[k])
                        v = m.vert.copy()
                        for c in range(3):
                            v[:, c] = (((M[c, 0] * base[:, 0] + M[c, 1] * base[:, 1]) + M[c, 2] * base[:, 2]) + float(t[k, c])).astype(f32)
                        verts.append(v)
                        faces.append(m.faces + 5 * k)
                    if int(f.get("connect", 0)) != 0:
                        faces.append(np.stack([5 * np.arange(len(t) - 1), 5 * np.arange(1, len(t))], 1).astype(np.uint32))
                    m = Mesh(np.concatenate(verts) if verts else np.zeros((0, 9), f32),
                             np.concatenate(faces) if faces else np.zeros((0, 2), np.uint32), 2, True, name)
            elif kind == "lines":
                m = Mesh.Lines(pts(), color, np.asarray(f["segs"], np.int64).reshape(-1, 2) if "segs" in f else None)
            elif kind == "points":
                m = Mesh.Points(pts(), color)
            elif kind == "mesh":
                fs = int(f.get("face_size", 3))
                if not 1 <= fs <= 3:
                    raise RtoError(-6, "open_drawlist: mesh '%s': face_size must be 1, 2 or 3" % name)
                m = Mesh._from_points(pts(), color, (0, 0, 1), np.asarray(f["faces"], np.int64).reshape(-1, fs) if "faces" in f else None,
                                      fs, False, name)
                m.estimate = fs == 3
            else:
                raise RtoError(-6, "open_drawlist: mesh '%s' has unsupported type '%s'" % (name, kind))
            if m.faces is not None and len(m.faces) and int(np.asarray(m.faces, np.int64).max()) >= len(m.vert):
                raise RtoError(-6, "open_drawlist: mesh '%s': an index is out of range" % name)
            if "vert_color" in f:
                vc = np.asarray(f["vert_color"], f32).reshape(-1, 3)
                if len(vc) != len(m.vert):
                    raise RtoError(-6, "open_drawlist: mesh '%s': vert_color has the wrong size" % name)
                m.vert[:, 3:6] = vc
            m.name = name
            m.placed(vec3("rotation", (0, 0, 0)), vec3("translation", (0, 0, 0)), float(f32(f.get("scale", 1.0))))
            m.visible = int(f.get("visible", int(default_visible))) != 0
            m.unlit = int(f.get("unlit", 0)) != 0 or m.face_size != 3
            out.append(m)
        return out

    def desc(self):
        """(rto_mesh_desc, the arrays it points into)"""
        d = CMeshDesc()
        d.vert, d.n_verts = self.vert.ctypes.data, len(self.vert)
        d.faces = self.faces.ctypes.data if self.faces is not None else None
        d.n_faces = len(self.faces) if self.faces is not None else 0
        d.face_size, d.unlit, d.estimate_normals = self.face_size, int(self.unlit), int(self.estimate)
        for i in range(3):
            d.rotation[i], d.translation[i] = float(self.rotation[i]), float(self.translation[i])
        d.scale = float(self.scale)
        return d, (self.vert, self.faces)


class MeshSet:
    """rto_meshes: the visible meshes of `meshes`, in order, baked into world space with one BVH over them.  device: a GPU index,
    or None for a host-only set (trace_rays_host, info and download only)."""

    def __init__(self, meshes, device=0, _handle=None):
        if _handle is None:
            meshes = [m for m in meshes if m.visible]
            parts = [m.desc() for m in meshes]
            arr = (CMeshDesc * max(1, len(parts)))(*[p[0] for p in parts])
            _handle = C.c_void_p(None)
            check(lib().rto_meshes_create(arr, len(parts), -1 if device is None else int(device), C.byref(_handle)))
        self._h = _handle
        self.device = device
        i = CMeshesInfo()
        check(lib().rto_meshes_get_info(self._h, C.byref(i)))
        self.triangles, self.segments, self.points, self.nodes = i.triangles, i.segments, i.points, i.nodes
        self.device_bytes = i.device_bytes
        self.bounds = (np.array(list(i.lo), f32), np.array(list(i.hi), f32))

    @staticmethod
    def load(path, device=0):
        """rto_meshes_load: an .obj or a drawlist .npz; a list of paths is concatenated in order (rto_meshes_load_files)"""
        paths = [path] if isinstance(path, (str, bytes)) else list(path)
        arr = (C.c_char_p * max(1, len(paths)))(*[p if isinstance(p, bytes) else str(p).encode() for p in paths])
        h = C.c_void_p(None)
        check(lib().rto_meshes_load_files(arr, len(paths), -1 if device is None else int(device), C.byref(h)))
        return MeshSet(None, device, _handle=h)

    @property
    def n_prims(self):
        return self.triangles + self.segments + self.points

    def download(self):
        """(prims [n, 32], nodes [nodes, 8]) float32: what the set holds (layouts: csrc/rto_mesh_trace.h)"""
        prims, nodes = np.zeros((self.n_prims, 32), f32), np.zeros((self.nodes, 8), f32)
        check(lib().rto_meshes_download(self._h, prims.ctypes.data, nodes.ctypes.data))
        return prims, nodes

    def trace_rays_host(self, origins, dirs, line_spread=0.0, point_spread=0.0, background=1.0):
        """rto_meshes_trace_rays_host: numpy [n, 3] rays -> (t_hit [n], rgb [n, 3]) on the CPU, by the kernels' own code"""
        o, d = np.ascontiguousarray(origins, f32).reshape(-1, 3), np.ascontiguousarray(dirs, f32).reshape(-1, 3)
        if o.shape != d.shape:
            raise RtoError(-1, "trace_rays_host: origins and dirs differ in shape")
        t, rgb = np.empty(len(o), f32), np.empty((len(o), 3), f32)
        r = CMeshRays()
        r.origins, r.dirs, r.n = o.ctypes.data, d.ctypes.data, len(o)
        r.line_spread, r.point_spread, r.background = float(line_spread), float(point_spread), float(background)
        check(lib().rto_meshes_trace_rays_host(self._h, C.byref(r), t.ctypes.data, rgb.ctypes.data))
        return t, rgb

    def close(self):
        if getattr(self, "_h", None):
            lib().rto_meshes_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MeshParams(LayerParams):
    """rto_mesh_params: line_px, point_px, background.  MeshParams(options) takes background = options.background_brightness."""
    CSTRUCT, DEFAULT = CMeshParams, "rto_mesh_params_default"

    def _load(self, c):
        self.line_px, self.point_px, self.background = c.line_px, c.point_px, c.background

    def to_c(self, merge=False):
        c = CMeshParams()
        c.line_px, c.point_px, c.background = float(self.line_px), float(self.point_px), float(self.background)
        c.flags = MESH_MERGE if merge else 0
        return c


def draw_mesh_layers(meshset, cams, params=None, depth=None, color=None, merge=False, stream=None):
    """rto_draw_mesh_layers: `meshset` ray-traced for the n cameras `cams` (one size) into depth [n, H, W] and color [n, H, W, 4],
    contiguous float32 torch tensors on the set's device -- allocated here when not given; depth=False / color=False for an output
    that is not wanted.  merge=True (RTO_MESH_MERGE): depth-test against what the given tensors hold.  Returns (depth, color),
    the inputs of RenderContext.set_layers.  Asynchronous on `stream` (default: torch's current stream); no sync."""
    from .volrend import _draw_layers
    return _draw_layers("draw_mesh_layers", lib().rto_draw_mesh_layers, meshset, cams, MeshParams() if params is None else params,
                        depth, color, merge, stream)


def trace_mesh_rays(meshset, origins, dirs, line_spread=0.0, point_spread=0.0, background=1.0, t_hit=None, rgb=None, stream=None):
    """rto_meshes_trace_rays: n rays (origins / dirs [n, 3]: contiguous float32 torch tensors on the set's device, or numpy arrays,
    copied over) -> (t_hit [n], rgb [n, 3]), which render_rays takes as t_max and background.  Asynchronous on `stream`."""
    import torch
    from .volrend import _ray_tensor, _stream_ptr
    device = torch.device("cuda", meshset.device)
    n = int(origins.shape[0])
    o = _ray_tensor(origins, "origins", 3, n, device)
    d = _ray_tensor(dirs, "dirs", 3, n, device)
    t = torch.empty((n,), dtype=torch.float32, device=device) if t_hit is None else _ray_tensor(t_hit, "t_hit", 0, n, device)
    c = torch.empty((n, 3), dtype=torch.float32, device=device) if rgb is None else _ray_tensor(rgb, "rgb", 3, n, device)
    if n == 0:
        return t, c
    if stream is None:
        stream = torch.cuda.current_stream(device)
    r = CMeshRays()
    r.origins, r.dirs, r.n = o.data_ptr(), d.data_ptr(), n
    r.line_spread, r.point_spread, r.background = float(line_spread), float(point_spread), float(background)
    check(lib().rto_meshes_trace_rays(meshset._h, C.byref(r), C.c_void_p(t.data_ptr()), C.c_void_p(c.data_ptr()), _stream_ptr(stream)))
    return t, c
