"""Not gpu: the C-ABI surface of the environment light -- symbols, the mcpt_environment layout against the C compiler, argument errors with a
null device, the PFM reader against mcpt_write_pfm, render_scene's refusals of a bad map -- and the numpy restatement (env_ref) of maps
loaded through mcpt_read_pfm: its pdf integrates to 1, a 1x1 map is the uniform sphere, and its draws follow its pdf (chi-square).

The oracle's environment mode (an extension of oracle/mcpt_oracle.c, restated from include/mcpt.h), held to something outside itself: its
tables and draws are env_ref's bit for bit on the edge maps (tests/env_scenes.py) and test_gpu_env.py's map, at two light counts; its
frames meet the closed forms of a diffuse floor under a constant sky and under a band, and of a Phong plate under a constant sky; a frame
whose camera rays all miss is the float fold of Le; without an environment, or with an inactive one, nothing changes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import env_ref
import env_scenes
from conftest import ROOT, SCENES

ERR_IO, ERR_PARSE, ERR_ARG, ERR_NO_DEVICE = -1, -2, -3, -4
NAMES = ["mcpt_device_set_environment", "mcpt_device_get_environment", "mcpt_environment_eval", "mcpt_environment_sample", "mcpt_read_pfm",
         "mcpt_multi_set_environment"]


def _null_device_rc(mcpt):
    return ERR_NO_DEVICE if mcpt.device_count() <= 0 else ERR_ARG


def test_environment_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "} mcpt_environment;" in hdr


def test_environment_layout_matches_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [n for n, _ in _lib.Environment._fields_]
    assert fields == ["width", "height", "rgb", "scale", "flags", "reserved"]
    src = tmp_path / "layout_env.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n  printf(\"%zu\\n\", sizeof(mcpt_environment));\n"
                   + "".join("  printf(\"%%zu\\n\", offsetof(mcpt_environment, %s));\n" % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout_env"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(_lib.Environment) == 32
    for i, f in enumerate(fields):
        assert out[1 + i] == getattr(_lib.Environment, f).offset, f


def _env(mcpt, w, h, texels, scale=1.0, flags=0, reserved=0):
    tex = np.ascontiguousarray(np.asarray(texels, dtype=np.float32).reshape(-1))
    e = mcpt.Environment(w, h, tex.ctypes.data_as(C.POINTER(C.c_float)), scale, flags, reserved)
    return e, tex


BAD = [dict(w=0, h=1), dict(w=1, h=0), dict(w=-2, h=1), dict(v=float("nan")), dict(v=float("inf")), dict(v=-1e-30), dict(scale=0.0),
       dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(flags=1), dict(reserved=3)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join("%s=%s" % kv for kv in b.items()) for b in BAD])
def test_argument_errors_with_a_null_device(mcpt, bad):
    L = mcpt.lib()
    w, h = bad.get("w", 2), bad.get("h", 2)
    vals = np.ones(max(w, 1) * max(h, 1) * 3)
    vals[1] = bad.get("v", 1.0)
    e, tex = _env(mcpt, w, h, vals, bad.get("scale", 1.0), bad.get("flags", 0), bad.get("reserved", 0))
    assert L.mcpt_device_set_environment(None, C.byref(e)) == ERR_ARG
    assert L.mcpt_multi_set_environment(None, C.byref(e)) == ERR_ARG


def test_valid_arguments_with_a_null_device(mcpt):
    L = mcpt.lib()
    e, tex = _env(mcpt, 2, 1, [0.5, 0.25, 0.0, 0.0, 0.0, 0.0])       # (an all-zero map is valid: inactive)
    rc = _null_device_rc(mcpt)
    assert L.mcpt_device_set_environment(None, C.byref(e)) == rc
    assert L.mcpt_device_set_environment(None, None) == rc
    assert L.mcpt_multi_set_environment(None, C.byref(e)) == rc
    w, hh, s, z = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
    assert L.mcpt_device_get_environment(None, C.byref(w), C.byref(hh), C.byref(s), C.byref(z)) == rc
    d = np.zeros(3)
    rgb = np.zeros(3)
    D = C.POINTER(C.c_double)
    assert L.mcpt_environment_eval(None, d.ctypes.data_as(D), 1, rgb.ctypes.data_as(D)) == rc
    assert L.mcpt_environment_eval(None, None, 1, rgb.ctypes.data_as(D)) == ERR_ARG
    pix = np.zeros(1, dtype=np.int32)
    I = C.POINTER(C.c_int32)
    pdf = np.zeros(1)
    args = (pix.ctypes.data_as(I), pix.ctypes.data_as(I))
    assert L.mcpt_environment_sample(None, 1, *args, 0, 1, d.ctypes.data_as(D), pdf.ctypes.data_as(D), rgb.ctypes.data_as(D)) == rc
    assert L.mcpt_environment_sample(None, 1, *args, -1, 1, d.ctypes.data_as(D), pdf.ctypes.data_as(D), rgb.ctypes.data_as(D)) == ERR_ARG


def test_pfm_round_trip_and_orientation(mcpt, tmp_path):
    rng = np.random.default_rng(1)
    img = rng.random((5, 7, 3)) * 10.0
    img[0, 0] = (1.0, 2.0, 3.0)             # top-left texel
    p = str(tmp_path / "m.pfm")
    mcpt.write_pfm(p, img)
    raw = open(p, "rb").read()
    assert raw.startswith(b"PF\n7 5\n-1.0\n")
    body = np.frombuffer(raw[len(b"PF\n7 5\n-1.0\n"):], dtype="<f4").reshape(5, 7, 3)
    assert np.array_equal(body[-1, 0], np.float32([1.0, 2.0, 3.0]))       # stored bottom row first: the top row comes last
    got = mcpt.read_pfm(p)
    assert got.dtype == np.float32 and got.shape == (5, 7, 3)
    assert np.array_equal(got, img.astype(np.float32))
    assert np.array_equal(got[0, 0], np.float32([1.0, 2.0, 3.0]))
    L = mcpt.lib()
    w, h = C.c_int32(), C.c_int32()
    small = np.zeros(10, dtype=np.float32)
    assert L.mcpt_read_pfm(p.encode(), C.byref(w), C.byref(h), small.ctypes.data_as(C.POINTER(C.c_float)), small.size) == ERR_ARG
    assert L.mcpt_read_pfm(str(tmp_path / "none.pfm").encode(), C.byref(w), C.byref(h), None, 0) == ERR_IO
    (tmp_path / "bad.pfm").write_bytes(b"Pf\n2 2\n-1.0\n" + b"\0" * 16)
    assert L.mcpt_read_pfm(str(tmp_path / "bad.pfm").encode(), C.byref(w), C.byref(h), None, 0) == ERR_PARSE
    # a big-endian file (positive scale) reads the same values
    (tmp_path / "be.pfm").write_bytes(b"PF\n7 5\n1.0\n" + img[::-1].astype(">f4").tobytes())
    assert np.array_equal(mcpt.read_pfm(str(tmp_path / "be.pfm")), img.astype(np.float32))


def _loaded(mcpt, tmp_path, m, name="map.pfm"):
    """an (H, W, 3) map as a caller loads one: written as a PFM, read back through mcpt_read_pfm"""
    p = str(tmp_path / name)
    mcpt.write_pfm(p, np.asarray(m, dtype=np.float64))
    return mcpt.read_pfm(p)


def _band_map(W=64, H=32, seed=3):
    rng = np.random.default_rng(seed)
    m = rng.random((H, W, 3)) * 4.0
    m[:, 5:9] *= 30.0                      # a bright strip
    m[H // 2:, :] *= 0.01                   # a dim lower hemisphere
    m[3, :] = 0.0                           # a black row (never drawn)
    return m


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (32, 64), (7, 5)])
def test_pdf_integrates_to_one(mcpt, tmp_path, shape):
    rng = np.random.default_rng(sum(shape))
    e = env_ref.EnvRef(_loaded(mcpt, tmp_path, rng.random(shape + (3,)) + 0.1), scale=2.5)
    assert (e.H, e.W) == shape
    total = float((e.pdf(*np.indices(shape)) * e.omega[:, None]).sum())
    assert abs(total - 1.0) < 1e-12
    assert abs(e.omega.sum() * e.W - 4.0 * np.pi) < 1e-12      # the rows cover the sphere


def test_constant_map_is_the_uniform_sphere(mcpt, tmp_path):
    e = env_ref.EnvRef(_loaded(mcpt, tmp_path, np.array([[[0.3, 0.6, 0.9]]])), scale=2.0)
    u = [np.random.default_rng(i).random(4000) for i in range(4)]
    i, j, d, pdf, rgb = e.sample_u(*u)
    assert np.all(i == 0) and np.all(j == 0)
    assert np.allclose(pdf, 1.0 / (4.0 * np.pi), rtol=0, atol=1e-15)
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-14)
    assert np.array_equal(rgb, np.tile(2.0 * np.float32([0.3, 0.6, 0.9]).astype(np.float64), (4000, 1)))
    assert abs(d[:, 1].mean()) < 0.05 and abs(d[:, 0].mean()) < 0.05


def test_draws_follow_the_pdf_chi_square(mcpt, tmp_path):
    e = env_ref.EnvRef(_loaded(mcpt, tmp_path, _band_map(16, 8)), scale=1.0)
    n = 200000
    rng = np.random.default_rng(7)
    i, j, d, pdf, rgb = e.sample_u(*(rng.random(n) for _ in range(4)))
    # the draw's own texel is the lookup's texel (away from borders), and its pdf the texel's
    ii, jj = e.texel_of(d)
    assert (ii == i).mean() > 0.999 and (jj == j).mean() > 0.999
    assert np.array_equal(pdf, e.lum[i, j] / e.Z)
    assert not np.any(i == 3)
    counts = np.bincount(i * e.W + j, minlength=e.H * e.W).astype(np.float64)
    expect = (e.lum * e.omega[:, None] / e.Z).reshape(-1) * n
    keep = expect > 5
    chi2 = float((((counts - expect) ** 2 / np.where(keep, expect, 1.0))[keep]).sum())
    dof = int(keep.sum()) - 1
    assert chi2 < dof + 6.0 * np.sqrt(2.0 * dof), (chi2, dof)
    assert counts[~keep].sum() <= expect[~keep].sum() + 6.0 * np.sqrt(expect[~keep].sum() + 1.0)


def test_lookup_rows_and_columns(mcpt, tmp_path):
    e = env_ref.EnvRef(_loaded(mcpt, tmp_path, _band_map(8, 4)))
    assert e.c[2] > 0.0 and e.c[3] < 0.0                 # c[2] = cos(pi / 2) rounds to 6.1e-17: y = 0 lies in row 2 (c[3] < 0 <= c[2])
    # straight up: row 0; straight down: the last row; the horizon: row 2; the +x axis: column 0; phi just under 2 pi: the last column
    i, j = e.texel_of([[0, 1, 0], [0, -1, 0], [1, 0, 0], [1, 0, -1e-9]])
    assert list(i) == [0, 3, 2, 2]
    assert list(j) == [0, 0, 0, 7]


def test_render_scene_refuses_a_bad_map_before_writing(mcpt, tmp_path):
    L = mcpt.lib()
    from montecarlopathtracing_amd import _lib
    o = _lib.RenderSceneOptions()
    o.quiet = 1
    prefix = str(tmp_path / "out")
    o.output_prefix = prefix.encode()
    bad = tmp_path / "bad.pfm"
    bad.write_bytes(b"P5\n2 2\n255\n" + bytes(4))
    neg = str(tmp_path / "neg.pfm")
    mcpt.write_pfm(neg, -np.ones((2, 2, 3)))
    ok = str(tmp_path / "ok.pfm")
    mcpt.write_pfm(ok, np.ones((2, 2, 3)))
    args = (SCENES.encode(), b"cornell-box", 1, C.byref(o), C.sizeof(o), None)
    assert L.mcpt_render_scene_env(*args, str(tmp_path / "none.pfm").encode(), 1.0, None) == ERR_IO
    assert L.mcpt_render_scene_env(*args, str(bad).encode(), 1.0, None) == ERR_PARSE
    assert L.mcpt_render_scene_env(*args, neg.encode(), 1.0, None) == ERR_ARG
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert L.mcpt_render_scene_env(*args, ok.encode(), scale, None) == ERR_ARG
    assert not os.path.exists(prefix + "-SPP1.png")


# ---------------------------------------------------------------------------------------------------------------- the oracle's environment
ORACLE_MAPS = dict(env_scenes.EDGE_MAPS, **{"sky-map": env_scenes.SKIES["map"]})
OW, OH = 48, 27


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _off_column_borders(d, W):
    phi = np.mod(np.arctan2(d[:, 2], d[:, 0]), 2 * np.pi) * W / (2 * np.pi)
    return np.abs(phi - np.round(phi)) * (2 * np.pi / W) >= 1e-12


@pytest.fixture(scope="module")
def env_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("env_scenes")) + os.sep
    env_scenes.open_scene(d, "open_nl0", 0, OW, OH)
    env_scenes.open_scene(d, "open_nl1", 1, OW, OH)
    return d


@pytest.mark.parametrize("scene", ["open_nl0", "open_nl1"])
@pytest.mark.parametrize("name", sorted(ORACLE_MAPS))
def test_oracle_tables_and_draws_are_the_restatement(oracle, env_dir, scene, name):
    rgb, scale = ORACLE_MAPS[name]
    osc = oracle.OracleScene(env_dir + scene)
    assert osc.num_lights == int(scene[-1])
    ref = env_ref.EnvRef(rgb, scale)
    assert ref.Z > 0
    assert osc.set_environment(rgb, scale) == ref.Z
    rng = np.random.default_rng(len(name))
    n = 2000
    pix = rng.integers(0, OW * OH, size=n).astype(np.int32)
    ks = rng.integers(0, 1000, size=n).astype(np.int32)
    dirs = [rng.normal(size=(2000, 3)), [[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, 1], [-1, 0, 0], [0, 0, -1], [1, 0, -1e-9]]]
    for depth in (0, 5):
        d, pdf, le = osc.env_sample(9, pix, ks, depth)
        i, j, dr, pr, lr = ref.sample_u(*env_ref.vertex_uniforms(9, pix, ks, depth, osc.num_lights))
        assert np.array_equal(_bits(pdf), _bits(pr)) and np.array_equal(_bits(le), _bits(lr))
        assert np.abs(d - dr).max() <= 1e-15
        assert np.all(ref.lum[i, j] > 0) and np.all(np.isfinite(pdf) & (pdf > 0)) and np.isfinite(le).all()
        dirs.append(d)
    dirs = np.concatenate(dirs)
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    keep = _off_column_borders(dirs, ref.W)
    assert np.array_equal(_bits(osc.env_eval(dirs)[keep]), _bits(ref.eval(dirs)[keep]))
    osc.close()


def test_oracle_without_an_environment_is_unchanged(oracle):
    osc = oracle.OracleScene(SCENES + "cornell-box", texture_dir=SCENES, width=32, height=18)
    st0 = oracle.Stats()
    ref = osc.render(2, seed=3, stats=st0)
    strided = osc.render_strided(2, 3, 4, faithful_cost=False)
    sample = osc.sample_radiance(3, 9, 16, 1)
    fields = [f for f, _ in oracle.Stats._fields_]
    assert st0.env_shadow == st0.env_shadow_clear == st0.env_escape_specular == st0.env_escape_transmission == st0.camera_miss == 0
    with pytest.raises(ValueError):
        osc.env_eval(np.array([[0.0, 1.0, 0.0]]))
    # an inactive (all-black) map is no environment; a cleared one neither
    assert osc.set_environment(np.zeros((4, 8, 3))) == 0.0
    st1 = oracle.Stats()
    assert np.array_equal(_bits(osc.render(2, seed=3, stats=st1)), _bits(ref))
    assert [getattr(st1, f) for f in fields] == [getattr(st0, f) for f in fields]
    assert osc.set_environment(*env_scenes.SKIES["map"]) > 0
    lit = osc.render(2, seed=3)
    assert not np.array_equal(_bits(lit), _bits(ref))
    # the CPU baseline's entry points ignore the environment
    assert np.array_equal(_bits(osc.render_strided(2, 3, 4, faithful_cost=False)), _bits(strided))
    assert osc.set_environment(None) == 0.0
    st2 = oracle.Stats()
    assert np.array_equal(_bits(osc.render(2, seed=3, stats=st2)), _bits(ref))
    assert [getattr(st2, f) for f in fields] == [getattr(st0, f) for f in fields]
    assert np.array_equal(_bits(osc.sample_radiance(3, 9, 16, 1)), _bits(sample))
    with pytest.raises(ValueError):
        osc.set_environment(np.full((2, 2, 3), -1.0))
    osc.close()


def _z(img, expect):
    x = img.reshape(-1, 3)
    m = x.mean(axis=0)
    s = x.std(axis=0, ddof=1) / np.sqrt(x.shape[0])
    return np.abs(m - expect) / np.maximum(s, 1e-300)


def test_oracle_diffuse_floor_under_a_constant_sky(oracle, tmp_path):
    rho, L = 0.5, np.array([1.0, 2.0, 0.5])
    env_scenes.floor_scene(str(tmp_path), "floor", (rho, rho, rho))
    osc = oracle.OracleScene(str(tmp_path / "floor"))
    assert osc.num_lights == 0
    assert np.all(osc.render(4, seed=1) == 0.0)                            # no lights, no sky: black
    osc.set_environment(L)
    st = oracle.Stats()
    img = osc.render(256, seed=2, stats=st)
    z = _z(img, rho * L)
    assert np.all(z < 5.0), z
    # every shadow ray sees the sky; nothing escapes but diffuse bounces (which add nothing); every camera ray hits the floor
    assert st.env_shadow > 0.4 * st.samples and st.env_shadow_clear == st.env_shadow == st.rays_shadow
    assert st.env_escape_specular == st.env_escape_transmission == st.camera_miss == 0
    osc.close()


def test_oracle_diffuse_floor_under_a_band(oracle, tmp_path):
    """test_gpu_env.py::test_diffuse_floor_under_a_band on the oracle"""
    rho = 0.8
    W_, H_ = 16, 8
    m = np.zeros((H_, W_, 3))
    m[1, 3:6] = [[4.0, 2.0, 1.0], [1.0, 1.0, 1.0], [0.5, 3.0, 2.0]]
    env_scenes.floor_scene(str(tmp_path), "floor", (rho, rho, rho))
    osc = oracle.OracleScene(str(tmp_path / "floor"))
    osc.set_environment(m)
    img = osc.render(512, seed=3)
    t0, t1 = np.pi * 1 / H_, np.pi * 2 / H_
    dphi = 2 * np.pi / W_
    expect = rho / np.pi * m[1, 3:6].sum(axis=0) * dphi * (np.sin(t1) ** 2 - np.sin(t0) ** 2) / 2
    z = _z(img, expect)
    assert np.all(z < 5.0), (z, img.reshape(-1, 3).mean(axis=0), expect)
    osc.close()


def test_oracle_phong_plate_under_a_constant_sky(oracle, tmp_path):
    """Kd = 0, Ks = 0.5: the light sample adds nothing and every bounce is SPECULAR; a bounce ray leaves the scene whichever way it goes
    and brings Ks * L / 0.6 with probability 0.6 -- Ks * L"""
    ks, L = 0.5, np.array([1.0, 2.0, 0.5])
    env_scenes.floor_scene(str(tmp_path), "plate", (0, 0, 0), ks=(ks, ks, ks), ns=20)
    osc = oracle.OracleScene(str(tmp_path / "plate"))
    osc.set_environment(L)
    st = oracle.Stats()
    img = osc.render(256, seed=4, stats=st)
    z = _z(img, ks * L)
    assert np.all(z < 5.0), (z, img.reshape(-1, 3).mean(axis=0))
    assert st.env_escape_specular == st.rays_bounce > 0.5 * st.samples
    assert st.env_escape_transmission == st.camera_miss == 0
    osc.close()


def _fold(x, n):
    acc = np.float32(0.0)
    for _ in range(n):
        acc = np.float32(np.float64(acc) + x / n)
    return np.float64(acc)


def test_oracle_camera_misses_are_the_folded_sky(oracle, tmp_path):
    W_, H_, N_ = 48, 27, 8
    env_scenes.floor_scene(str(tmp_path), "up", (0.5, 0.5, 0.5), width=W_, height=H_, look_up=True)
    osc = oracle.OracleScene(str(tmp_path / "up"))
    rgb, scale = env_scenes.SKIES["map"]
    osc.set_environment(rgb, scale)
    rays = osc.primary_rays()
    face = osc.trace_closest(rays)[0]
    assert np.all(face < 0)
    le = osc.env_eval(rays[:, 3:])
    assert np.array_equal(_bits(le), _bits(env_ref.EnvRef(rgb, scale).eval(rays[:, 3:])))
    want = np.array([[_fold(x, N_) for x in row] for row in le]).reshape(H_, W_, 3)
    for faithful in (False, True):
        st = oracle.Stats()
        img = osc.render(N_, seed=4, faithful_cost=faithful, stats=st)
        assert np.array_equal(_bits(img), _bits(want)), faithful
        assert st.camera_miss == st.samples == W_ * H_ * N_ and st.shade_calls == 0
    assert np.array_equal(_bits(osc.sample_radiance(4, 5, 7, 3)), _bits(le[5 * W_ + 7]))
    osc.close()
