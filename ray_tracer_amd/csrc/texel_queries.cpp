// texel_queries.cpp — see texel_queries.h. Host only: compiled into the library by hipcc and into tests/texels_check.cpp by g++.
#include "texel_queries.h"

#include <cstring>
#include <vector>

#include "rt_texels.h"

namespace {
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
bool size_ok(uint32_t v) { return v >= 1u && v <= (uint32_t)RT_TEXEL_MAX_SIZE; }

// The object's triangles as RootInfo.triFirst / triTotal say them: the leaves' ranges under its root, one contiguous run
bool object_triangles(const RtSceneArrays& s, uint32_t object, uint32_t* first, uint32_t* total) {
    const uint32_t root = s.objects[object].bvhIndex;
    if (root >= s.bvhNodeCount) return false;
    std::vector<uint32_t> st(1, root);
    size_t visited = 0;
    uint64_t lo = ~0ull, hi = 0, sum = 0;
    while (!st.empty()) {
        const uint32_t nidx = st.back();
        st.pop_back();
        if (nidx >= s.bvhNodeCount || ++visited > (size_t)s.bvhNodeCount + 1) return false;
        const BVHNode& b = s.bvhNodes[nidx];
        if (b.triCount) {
            if ((uint64_t)b.index + b.triCount > s.triangleCount) return false;
            lo = b.index < lo ? b.index : lo;
            hi = (uint64_t)b.index + b.triCount > hi ? (uint64_t)b.index + b.triCount : hi;
            sum += b.triCount;
        } else {
            st.push_back(b.index);
            st.push_back(b.index + 1);
        }
    }
    if (sum == 0 || sum != hi - lo) return false;
    *first = (uint32_t)lo;
    *total = (uint32_t)sum;
    return true;
}

// (what RT_OBJ_FWD_IDENTITY says on the device: the rows of the matrix are exactly the identity's)
bool rows_identity(const float* m) {
    bool is = true;
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 3; r++) is = is && m[c * 4 + r] == (r == c ? 1.f : 0.f);
    return is;
}

rt_vec3 v3(const float* p) { return rt_v3(p[0], p[1], p[2]); }
}  // namespace

std::string check_texel_size(const char* fn, uint32_t width, uint32_t height) {
    if (!size_ok(width) || !size_ok(height))
        return std::string(fn) + ": a map of " + std::to_string(width) + " x " + std::to_string(height) + " texels; width and height must be in 1 .. 8192";
    return "";
}

std::string check_texel_bake(const char* fn, bool sceneUploaded, const void* out, uint32_t object, uint32_t objectCount, uint32_t width,
                             uint32_t height, uint32_t triTotal) {
    const std::string f(fn);
    if (!sceneUploaded) return f + " before rt_upload_scene";
    if (!out) return f + ": the output is required";
    if (object >= objectCount) return f + ": object " + std::to_string(object) + " of " + std::to_string(objectCount);
    const std::string size = check_texel_size(fn, width, height);
    if (!size.empty()) return size;
    if (triTotal == 0xffffffffu) return f + ": the triangles of object " + std::to_string(object) + "'s mesh are not one contiguous range";
    return "";
}

std::string check_lightmap(const char* fn, const RtIrradianceParams* params, uint32_t dilatePasses, const void* fill) {
    const std::string f(fn);
    if (!params) return f + ": the params are required";
    if (params->progressive) return f + ": one shot; progressive refinement goes through rt_texels_compact and rt_query_irradiance";
    if (dilatePasses > (uint32_t)RT_TEXEL_MAX_PASSES) return f + ": at most 254 dilation passes";
    if (!fill) return f + ": the fill plane is required";
    return "";
}

std::string check_texel_pass(const char* fn, bool allRequired, uint64_t nTexels, uint32_t nCovered, uint32_t passes) {
    const std::string f(fn);
    if (!allRequired) return f + ": every array is required";
    if (nTexels == 0 || nTexels > (uint64_t)RT_TEXEL_MAX_SIZE * RT_TEXEL_MAX_SIZE) return f + ": " + std::to_string(nTexels) + " texels; a map has 1 .. 8192 x 8192";
    if (nCovered > nTexels) return f + ": " + std::to_string(nCovered) + " covered texels of " + std::to_string(nTexels);
    if (passes > (uint32_t)RT_TEXEL_MAX_PASSES) return f + ": at most 254 dilation passes";
    return "";
}

uint32_t texel_groups(uint64_t n, uint32_t threads) { return (uint32_t)((n + threads - 1) / threads); }

ScanLevels scan_levels(uint64_t n) {
    ScanLevels s;
    memset(&s, 0, sizeof s);
    uint64_t count = n ? n : 1, offset = 0;
    for (;;) {
        const uint64_t sums = (count + RT_TEXEL_SCAN_BLOCK - 1) / RT_TEXEL_SCAN_BLOCK;
        s.count[s.levels] = count;
        s.offset[s.levels] = offset;
        s.levels++;
        offset += sums;
        if ((count == 1 && s.levels >= 2) || s.levels == RT_TEXEL_MAX_LEVELS) break;
        count = sums;
    }
    s.elems = offset;
    return s;
}

TexelScratch texel_scratch(uint32_t nTris, uint32_t width, uint32_t height) {
    const size_t n = (size_t)width * height, t = (size_t)nTris + 1;
    TexelScratch s;
    s.stats = 0;
    s.owner = 256;
    s.overlapped = s.owner + align256(4 * n);
    s.counts = s.overlapped + align256(n);
    s.offsets = s.counts + align256(4 * t);
    s.sums = s.offsets + align256(8 * t);
    s.bytes = s.sums + align256(8 * (size_t)scan_levels(t).elems);
    return s;
}

LightmapScratch lightmap_scratch(uint32_t width, uint32_t height) {
    const size_t n = (size_t)width * height;
    LightmapScratch s;
    s.texels = 0;
    s.points = align256(48 * n);
    s.normals = s.points + align256(12 * n);
    s.index = s.normals + align256(12 * n);
    s.count = s.index + align256(4 * n);
    s.values = s.count + 256;
    s.bytes = s.values + align256(16 * n);
    return s;
}

extern "C" {

int rt_texels_exhaustive_host(const RtSceneArrays* s, uint32_t object, uint32_t width, uint32_t height, RtTexel* texels, RtTexelStats* stats) {
    if (!s || !texels) return -1;
    if (object >= s->objectCount || !size_ok(width) || !size_ok(height)) return -1;
    uint32_t first, total;
    if (!object_triangles(*s, object, &first, &total)) return -1;
    for (uint32_t t = first; t < first + total; t++)
        if (s->triangles[t].v0 >= s->triPointCount || s->triangles[t].v1 >= s->triPointCount || s->triangles[t].v2 >= s->triPointCount) return -1;
    const size_t n = (size_t)width * height;
    std::vector<uint32_t> owner(n, RT_TEXEL_EMPTY);
    std::vector<uint8_t> overlapped(n, 0);
    RtTexelStats st{0, 0, 0, 0};
    const auto uv_of = [&](uint32_t t, float* uv) {
        const Triangle& tr = s->triangles[t];
        const TrianglePoint &p0 = s->triPoints[tr.v0], &p1 = s->triPoints[tr.v1], &p2 = s->triPoints[tr.v2];
        uv[0] = p0.position[3]; uv[1] = p0.normal[3]; uv[2] = p1.position[3]; uv[3] = p1.normal[3]; uv[4] = p2.position[3]; uv[5] = p2.normal[3];
    };
    // ascending triangles: the first to cover a centre is its owner, any later one makes it overlapped
    for (uint32_t t = first; t < first + total; t++) {
        float uv[6];
        uv_of(t, uv);
        rt_texel_tri tri;
        if (!rt_texel_setup(uv, width, height, &tri)) { st.skippedTriangles++; continue; }
        rt_texel_box box;
        if (!rt_texel_bounds(&tri, width, height, &box)) continue;
        for (uint32_t y = box.y0; y <= box.y1; y++)
            for (uint32_t x = box.x0; x <= box.x1; x++) {
                if (!rt_texel_covers(&tri, x, y, nullptr, nullptr)) continue;
                const size_t i = (size_t)y * width + x;
                if (owner[i] == RT_TEXEL_EMPTY) owner[i] = t;
                else overlapped[i] = 1;
            }
    }
    const float* m = s->objects[object].transformMatrix;
    const rt_rows fwd = rt_rows_of(m);
    const bool identity = rows_identity(m);
    memset(texels, 0, n * sizeof(RtTexel));
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) {
            const size_t i = (size_t)y * width + x;
            const uint32_t t = owner[i];
            if (t == RT_TEXEL_EMPTY) continue;
            float uv[6];
            uv_of(t, uv);
            rt_texel_tri tri;
            int64_t e1 = 0, e2 = 0;
            (void)rt_texel_setup(uv, width, height, &tri);
            (void)rt_texel_covers(&tri, x, y, &e1, &e2);
            const Triangle& tr = s->triangles[t];
            const TrianglePoint &p0 = s->triPoints[tr.v0], &p1 = s->triPoints[tr.v1], &p2 = s->triPoints[tr.v2];
            rt_texel_record r;
            if (!rt_texel_make_record(e1, e2, tri.area, v3(p0.position), v3(p1.position), v3(p2.position), v3(p0.normal), v3(p1.normal), v3(p2.normal),
                                      &fwd, identity, &r)) {
                st.degenerateTexels++;
                continue;
            }
            RtTexel& o = texels[i];
            o.point[0] = r.point.x; o.point[1] = r.point.y; o.point[2] = r.point.z;
            o.state = overlapped[i] ? 3u : 1u;
            o.normal[0] = r.normal.x; o.normal[1] = r.normal.y; o.normal[2] = r.normal.z;
            o.triIndex = t;
            o.uv[0] = r.u; o.uv[1] = r.v;
            st.covered++;
            st.overlapped += overlapped[i] ? 1u : 0u;
        }
    if (stats) *stats = st;
    return 0;
}

int rt_dilate_texels_host(uint32_t width, uint32_t height, uint32_t passes, float* rgba, uint8_t* fill) {
    if (!rgba || !fill || !size_ok(width) || !size_ok(height) || passes > (uint32_t)RT_TEXEL_MAX_PASSES) return -1;
    const size_t n = (size_t)width * height;
    std::vector<float> other(4 * n);
    std::vector<uint8_t> otherFill(n);
    for (uint32_t k = 1; k <= passes; k++) {
        for (uint32_t y = 0; y < height; y++)
            for (uint32_t x = 0; x < width; x++) {
                const size_t i = (size_t)y * width + x;
                rt_dilate_texel(width, height, x, y, k, rgba, fill, &other[4 * i], &otherFill[i]);
            }
        memcpy(rgba, other.data(), 4 * n * sizeof(float));
        memcpy(fill, otherFill.data(), n);
    }
    return 0;
}

}  // extern "C"
