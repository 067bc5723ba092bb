"""Makes tests/golden/reference_struct_layout.json: sizeof and the field offsets of the reference's host structs
(src/vk_engine.h, compiled with the glm it vendors under third_party/glm), the numbers
tests/test_abi_smoke.py::test_structs_equal_the_references_own_header holds include/rt_amd.h to.
Only the numbers are stored; the header itself stays in the reference tree.

usage: python tools/reference_layout.py <reference tree> [out.json]"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {   # struct -> fields whose offsets are recorded
    "Sphere": ["position", "radius", "materialIndex"],
    "Triangle": ["v0", "v1", "v2", "frontOnly", "binormal", "tangent"],
    "TrianglePoint": ["position", "normal"],
    "RayMaterial": ["albedo", "emissionColor", "emissionStrength", "reflectance", "ior", "albedoIndex", "metalnessIndex", "alphaIndex", "bumpIndex"],
    "RenderObject": ["transformMatrix", "smoothShade", "bvhIndex", "materialIndex", "samplerIndex"],
    "BVHNode": ["boundsX", "boundsY", "boundsZ", "index", "triCount"],
    "CameraInfo": ["cameraRotation", "pos", "nearPlane", "aspectRatio", "fov"],
    "EnvironmentData": ["horizonColor", "zenithColor", "groundColor", "lightDir"],
    "RayTracerData": ["progressive", "singleRender", "debug", "raysPerPixel", "bounceLimit", "sphereCount", "objectCount", "triangleCap", "boxCap", "sampleLimit"],
    "PushConstants": ["camInfo", "environment", "rayTraceParams", "frameCount"],
}


def main():
    ref = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "reference_struct_layout.json")
    text = open(os.path.join(ref, "src", "vk_engine.h"), encoding="utf-8-sig").read()
    bodies = []
    for name in STRUCTS:
        m = re.search(r"^struct %s \{.*?^\};" % name, text, flags=re.S | re.M)
        if not m:
            raise SystemExit(f"struct {name} not found in the reference's header")
        bodies.append(m.group(0))
    prints = []
    for name, fields in STRUCTS.items():
        prints.append(f'std::printf("{name} sizeof %zu\\n", sizeof({name}));')
        for f in fields:
            prints.append(f'std::printf("{name} {f} %zu\\n", offsetof({name}, {f}));')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.cpp"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write("#include <sys/types.h>\n#include <cstddef>\n#include <cstdio>\n#include <glm/glm.hpp>\n" + "\n".join(bodies)
                     + "\nint main() {\n" + "\n".join(prints) + "\nreturn 0;\n}\n")
        subprocess.run(["g++", "-std=c++17", "-Wno-invalid-offsetof", "-I", os.path.join(ref, "third_party", "glm"), src, "-o", exe], check=True)
        lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    layout = {name: {"sizeof": None, "offsets": {}} for name in STRUCTS}
    for ln in filter(None, lines):
        name, field, value = ln.split()
        if field == "sizeof":
            layout[name]["sizeof"] = int(value)
        else:
            layout[name]["offsets"][field] = int(value)
    with open(out, "w") as fh:
        json.dump(layout, fh, indent=1)
        fh.write("\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
