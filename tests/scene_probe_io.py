"""The files of examples/scene_probe.cpp: a scene description written from a SceneBuilder.desc() (an abi.SrtSceneDesc), and
the flattened scene read back as {member name: Member}.  The formats are in the header of examples/scene_probe.cpp."""
import collections
import ctypes as C
import hashlib
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULT_OPTIONS = (1, 0, 1)  # srt_api.cpp's defaults of the tunables wf_hybrid, wf_resident_max, fast_div

Member = collections.namedtuple("Member", "count size data")  # count -1: a scalar (its value in data, as bytes)


def _array(count, ptr, itemsize, carried):
    """i64 count, i64 bytes, the bytes: a null pointer (or a count that is not positive) has none."""
    n = (count if carried is None else carried) * itemsize if ptr and count > 0 else 0
    return struct.pack("<qq", count, n) + (C.string_at(ptr, n) if n else b"")


def _world(desc, abi):
    out = b""
    if desc.world and desc.numWorld > 0:
        for w in range(desc.numWorld):
            it = desc.world[w]
            out += bytes(it)
            if it.nodes and it.numNodes > 0:
                out += C.string_at(it.nodes, it.numNodes * C.sizeof(abi.SrtBvhNode))
    return struct.pack("<qq", desc.numWorld, len(out)) + out


def write_scene(path, desc, abi, options=DEFAULT_OPTIONS, draws=0, carried={}):
    """desc's arrays in order, the caller-built nodes of a world item behind the item, the options, the draws to skip.
    carried: {"triangles": n} writes n elements of that array whatever its count says (a count no file can hold)."""
    def arr(count, name, ctype):
        return _array(getattr(desc, count), C.cast(getattr(desc, name), C.c_void_p).value, C.sizeof(ctype), carried.get(name))
    with open(path, "wb") as f:
        f.write(arr("numTriangles", "triangles", abi.SrtTriangleIn))
        f.write(arr("numSpheres", "spheres", abi.SrtSphereIn))
        f.write(arr("numPrims", "prims", abi.SrtPrimRef))
        f.write(_world(desc, abi))
        f.write(arr("numMaterials", "materials", abi.SrtMaterialIn))
        f.write(arr("numTextures", "textures", abi.SrtTextureIn))
        f.write(arr("numTexelBytes", "texels", C.c_uint8))
        f.write(struct.pack("<4i", *options, draws))


def read_flattened(path):
    """{name: Member} in the file's order; a refusal is the single member "error"."""
    b, at, out = open(path, "rb").read(), 0, collections.OrderedDict()
    while at < len(b):
        name = b[at + 1:at + 1 + b[at]].decode()
        at += 1 + b[at]
        count, size = struct.unpack_from("<qq", b, at)
        n = (1 if count < 0 else count) * size
        assert name not in out and at + 16 + n <= len(b), name
        out[name] = Member(count, size, b[at + 16:at + 16 + n])
        at += 16 + n
    return out


def digest(members):
    """What tests/golden/flatten_scenes.json keeps of a flattened scene: per vector its element count and the SHA-256 of its
    bytes, per scalar its value; of a refusal the text."""
    if "error" in members:
        return {"error": members["error"].data.decode()}
    return {k: struct.unpack("<i", m.data)[0] if m.count < 0 else [m.count, hashlib.sha256(m.data).hexdigest()] for k, m in members.items()}


def build(target="srt_scene_probe", scene_cpp=None):
    """make the probe (examples/<target>), or at the path `target` one that links another revision of srt_scene.cpp."""
    csrc = os.path.join(ROOT, "sexy-raytracer_amd", "csrc")
    if scene_cpp is None:
        subprocess.check_call(["make", "-C", csrc, "../../examples/" + target])
        return os.path.join(ROOT, "examples", target)
    probe = target[:-len("_san")] if target.endswith("_san") else target
    subprocess.check_call(["make", "-C", csrc, "SCENE_CPP=" + scene_cpp, "SCENE_PROBE=" + probe, target])
    return target


def flatten(exe, workdir, desc, abi, options=DEFAULT_OPTIONS, draws=0, carried={}, env=None):
    """The probe's `flatten` over one scene description: {name: Member}, and the milliseconds validateScene and flattenScene took."""
    src, dst = os.path.join(str(workdir), "scene.in"), os.path.join(str(workdir), "scene.out")
    write_scene(src, desc, abi, options, draws, carried)
    r = subprocess.run([exe, "flatten", src, dst], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout[-2000:]
    return read_flattened(dst), float(r.stdout.split("flatten_ms")[1].split()[0])


def validate(exe, workdir, desc, abi, carried={}, env=None):
    """The probe's `validate`: validateScene's message, empty for a valid scene."""
    src = os.path.join(str(workdir), "scene.in")
    write_scene(src, desc, abi, carried=carried)
    r = subprocess.run([exe, "validate", src], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.endswith("\n") and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout[-2000:]
    return r.stdout[:-1]
