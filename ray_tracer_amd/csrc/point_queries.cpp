// point_queries.cpp — see point_queries.h. Host only: compiled into the library by hipcc and into tests/point_queries_check.cpp by g++.
#include "point_queries.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <utility>

#include "rt_point_query.h"

namespace {
const double U32 = 5.9604644775390625e-8;   // 2^-24

// permanents of |M|'s minors: what inverse_error_unit (tests/brute_force.py) counts the cofactors' and the determinant's rounding with
double perm3(const double a[3][3]) {
    return a[0][0] * (a[1][1] * a[2][2] + a[1][2] * a[2][1]) + a[0][1] * (a[1][0] * a[2][2] + a[1][2] * a[2][0]) +
           a[0][2] * (a[1][0] * a[2][1] + a[1][1] * a[2][0]);
}
double perm_minor(const double A[4][4], int dropRow, int dropCol) {
    double m[3][3];
    for (int r = 0, rr = 0; r < 4; r++) {
        if (r == dropRow) continue;
        for (int c = 0, cc = 0; c < 4; c++) {
            if (c == dropCol) continue;
            m[rr][cc++] = A[r][c];
        }
        rr++;
    }
    return perm3(m);
}
double det3(const double a[3][3]) {
    return a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
}
double det_minor(const double A[4][4], int dropRow, int dropCol) {
    double m[3][3];
    for (int r = 0, rr = 0; r < 4; r++) {
        if (r == dropRow) continue;
        for (int c = 0, cc = 0; c < 4; c++) {
            if (c == dropCol) continue;
            m[rr][cc++] = A[r][c];
        }
        rr++;
    }
    return det3(m);
}

// the singular values of a 3x3 by one-sided Jacobi rotations of its columns (each to high relative accuracy): the smallest
double smallest_singular_value(const double m[3][3]) {
    double a[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) a[r][c] = m[r][c];
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int r = 0; r < 3; r++) { alpha += a[r][p] * a[r][p]; beta += a[r][q] * a[r][q]; gamma += a[r][p] * a[r][q]; }
                if (!(std::fabs(gamma) > 1e-17 * std::sqrt(alpha * beta))) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
                for (int r = 0; r < 3; r++) {
                    const double x = a[r][p], y = a[r][q];
                    a[r][p] = cs * x - sn * y;
                    a[r][q] = sn * x + cs * y;
                }
            }
        if (!rotated) break;
    }
    double least = std::numeric_limits<double>::infinity();
    for (int c = 0; c < 3; c++) least = std::min(least, std::sqrt(a[0][c] * a[0][c] + a[1][c] * a[1][c] + a[2][c] * a[2][c]));
    return least;
}

float round_down(double v) {   // the float at or below v (v >= 0)
    float f = (float)v;
    return (double)f > v ? std::nextafterf(f, 0.f) : f;
}
float round_up(double v) {     // the float at or above v (v >= 0)
    float f = (float)v;
    return (double)f < v ? std::nextafterf(f, std::numeric_limits<float>::infinity()) : f;
}

float4 f4(float x, float y, float z, float w) {
    float4 v;
    v.x = x; v.y = y; v.z = z; v.w = w;
    return v;
}
}  // namespace

std::string check_point_query(const char* fn, bool sceneUploaded, const RtPointBatch* points, const void* out) {
    const std::string f(fn);
    if (!sceneUploaded) return f + " before rt_upload_scene";
    if (!points) return f + ": the batch is NULL";
    if (points->n == 0) return "";
    if (!points->points || !out) return f + ": points and the output are required";
    if (points->n >= (uint32_t)RT_NEAREST_MAX_POINTS) return f + ": a batch of " + std::to_string(points->n) + " points does not fit the 30 bits of a slot id";
    return "";
}

PointShape point_shape(uint32_t n, uint32_t threads) {
    PointShape s;
    s.blocks = (uint32_t)(((uint64_t)n + threads - 1) / threads);
    s.pointBytes = (size_t)n * 3 * sizeof(float);
    s.limitBytes = (size_t)n * sizeof(float);
    s.outBytes = (size_t)n * sizeof(RtNearest);
    return s;
}

uint32_t nearest_stack(const char* fn, uint32_t maxLeafDepth, std::string* error) {
    if (maxLeafDepth <= (uint32_t)RT_NEAREST_STACK) return RT_NEAREST_STACK;
    if (maxLeafDepth <= (uint32_t)RT_NEAREST_STACK_DEEP) return RT_NEAREST_STACK_DEEP;
    if (error)
        *error = std::string(fn) + ": the scene's BVH has a leaf at depth " + std::to_string(maxLeafDepth) + ", beyond the " +
                 std::to_string((int)RT_NEAREST_STACK_DEEP) + " entries of the deepest k_nearest_points";
    return 0;
}

NearestPrune nearest_prune(const float* m, bool fwdIdentity) {
    if (fwdIdentity) return NearestPrune{1.f, 0.f};
    double M[4][4], A[4][4];   // row r, column c of the column-major m[c * 4 + r]
    bool finite = true;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            M[r][c] = (double)m[c * 4 + r];
            A[r][c] = std::fabs(M[r][c]);
            finite = finite && std::isfinite(M[r][c]);
        }
    if (!finite) return NearestPrune{0.f, 0.f};
    double m3[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m3[r][c] = M[r][c];
    const double s = smallest_singular_value(m3) * (1.0 - RT_NEAREST_SMIN_MARGIN);
    // det and permanent of the 4x4 by the first row
    double det = 0, pdet = 0;
    for (int c = 0; c < 4; c++) {
        det += ((c & 1) ? -1.0 : 1.0) * M[0][c] * det_minor(M, 0, c);
        pdet += A[0][c] * perm_minor(A, 0, c);
    }
    const double adet = std::fabs(det);
    if (!(adet > 0) || !std::isfinite(s)) return NearestPrune{0.f, 0.f};
    // rows 0..2 of the inverse: inverse[i][j] = cofactor(j, i) / det; E1[i][j] = perm(minor(j, i)) / |det| + |inverse[i][j]| (pdet / |det| + 1)
    double worst = 0;
    for (int i = 0; i < 3; i++) {
        double row = 0;
        for (int j = 0; j < 4; j++) {
            const double inv = std::fabs(det_minor(M, j, i)) / adet;
            const double e1 = perm_minor(A, j, i) / adet + inv * (pdet / adet + 1.0);
            row += 10.0 * e1 + 4.0 * inv;
        }
        worst = std::max(worst, row);
    }
    const double pad = std::sqrt(3.0) * U32 * worst;
    if (!std::isfinite(pad)) return NearestPrune{0.f, 0.f};
    return NearestPrune{round_down(std::max(s, 0.0)), round_up(pad)};
}

std::vector<float4> layout_nearest(const ObjectLayout& l, const RenderObject* o, uint32_t n, const std::vector<RootInfo>& rootOf) {
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float4> t((size_t)std::max(n, 1u) * 3, f4(0.f, 0.f, 0.f, 0.f));
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t flags = l.meta[i].w;
        const bool ident = (flags & RT_OBJ_FWD_IDENTITY) != 0u;
        const NearestPrune p = nearest_prune(o[i].transformMatrix, ident);
        const RootInfo& r = rootOf[o[i].bvhIndex];
        float lo[3] = {-inf, -inf, -inf}, hi[3] = {inf, inf, inf};
        if (ident) {
            for (int d = 0; d < 3; d++) { lo[d] = r.lo[d]; hi[d] = r.hi[d]; }
        } else if (flags & RT_OBJ_BOX) {
            const float4 &bl = l.box[2 * (size_t)i], &bh = l.box[2 * (size_t)i + 1];
            lo[0] = bl.x; lo[1] = bl.y; lo[2] = bl.z;
            hi[0] = bh.x; hi[1] = bh.y; hi[2] = bh.z;
        }
        // |M| |[v; 1]| over the root box (its largest is at the corner of the largest |coordinates|), and the world box itself
        double mag = 0;
        const float* m = o[i].transformMatrix;
        for (int d = 0; d < 3; d++) {
            double row = std::fabs((double)m[12 + d]);
            for (int k = 0; k < 3; k++) row += std::fabs((double)m[k * 4 + d]) * std::max(std::fabs((double)r.lo[k]), std::fabs((double)r.hi[k]));
            mag = std::max(mag, std::max(row, std::max(std::fabs((double)lo[d]), std::fabs((double)hi[d]))));
        }
        const float magF = std::isfinite(mag) ? round_up(mag) : inf;
        t[3 * (size_t)i] = f4(lo[0], lo[1], lo[2], p.sMin);
        t[3 * (size_t)i + 1] = f4(hi[0], hi[1], hi[2], p.padQ);
        t[3 * (size_t)i + 2] = f4(magF, 0.f, 0.f, 0.f);
    }
    return t;
}

// (the BVH only says which triangles a mesh has)
bool object_triangle_ranges(const RtSceneArrays& s, std::vector<TriangleRanges>* out) {
    std::vector<TriangleRanges>& rangesOf = *out;
    rangesOf.assign(s.objectCount, TriangleRanges());
    for (uint32_t i = 0; i < s.objectCount; i++) {
        const uint32_t root = s.objects[i].bvhIndex;
        if (root >= s.bvhNodeCount) return false;
        bool shared = false;
        for (uint32_t k = 0; k < i && !shared; k++)
            if (s.objects[k].bvhIndex == root) { rangesOf[i] = rangesOf[k]; shared = true; }
        if (shared) continue;
        std::vector<uint32_t> st(1, root);
        size_t visited = 0;
        while (!st.empty()) {
            const uint32_t nidx = st.back();
            st.pop_back();
            if (nidx >= s.bvhNodeCount || ++visited > (size_t)s.bvhNodeCount + 1) return false;
            const BVHNode& b = s.bvhNodes[nidx];
            if (b.triCount) {
                if ((uint64_t)b.index + b.triCount > s.triangleCount) return false;
                rangesOf[i].emplace_back(b.index, b.triCount);
            } else {
                st.push_back(b.index);
                st.push_back(b.index + 1);
            }
        }
        std::sort(rangesOf[i].begin(), rangesOf[i].end());
    }
    for (uint32_t t = 0; t < s.triangleCount; t++)
        if (s.triangles[t].v0 >= s.triPointCount || s.triangles[t].v1 >= s.triPointCount || s.triangles[t].v2 >= s.triPointCount) return false;
    return true;
}

// (what RT_OBJ_FWD_IDENTITY says on the device)
bool matrix_rows_identity(const float* m) {
    bool is = true;
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 3; r++) is = is && m[c * 4 + r] == (r == c ? 1.f : 0.f);
    return is;
}

extern "C" {

int rt_nearest_exhaustive_host(const RtSceneArrays* s, const RtPointBatch* points, RtNearest* out) {
    if (!s || !points) return -1;
    const uint32_t n = points->n;
    if (n == 0) return 0;
    if (!points->points || !out || n >= (uint32_t)RT_NEAREST_MAX_POINTS) return -1;
    std::vector<TriangleRanges> rangesOf;
    if (!object_triangle_ranges(*s, &rangesOf)) return -1;
    for (uint32_t i = 0; i < n; i++) {
        RtNearest r;
        memset(&r, 0, sizeof r);
        r.dst = RT_MISS_DST;
        const rt_vec3 q = rt_v3(points->points[(size_t)i * 3], points->points[(size_t)i * 3 + 1], points->points[(size_t)i * 3 + 2]);
        bool search;
        float best2 = rt_nearest_start(points->maxDist != nullptr, points->maxDist ? points->maxDist[i] : 0.f, &search);
        if (search) {
            rt_vec3 bestP = rt_v3(0.f, 0.f, 0.f);
            for (uint32_t k = 0; k < s->sphereCount; k++) {
                const Sphere& sp = s->spheres[k];
                if (!rt_sphere_is_surface(sp.radius)) continue;
                rt_vec3 p;
                const float d2 = rt_point_sphere(q, rt_v3(sp.position[0], sp.position[1], sp.position[2]), sp.radius, &p);
                if (d2 < best2) { best2 = d2; r.found = 1; r.isSphere = 1; r.objectIndex = k; bestP = p; }
            }
            for (uint32_t k = 0; k < s->objectCount; k++) {
                const float* m = s->objects[k].transformMatrix;
                const bool isIdent = matrix_rows_identity(m);
                for (const auto& range : rangesOf[k])
                    for (uint32_t t = range.first; t < range.first + range.second; t++) {
                        const Triangle& tr = s->triangles[t];
                        const float *pa = s->triPoints[tr.v0].position, *pb = s->triPoints[tr.v1].position, *pc = s->triPoints[tr.v2].position;
                        rt_vec3 a = rt_v3(pa[0], pa[1], pa[2]), b = rt_v3(pb[0], pb[1], pb[2]), c = rt_v3(pc[0], pc[1], pc[2]);
                        if (!isIdent) { a = rt_xform_point(m, a); b = rt_xform_point(m, b); c = rt_xform_point(m, c); }
                        float u, v;
                        const float d2 = rt_point_triangle(q, a, b, c, &u, &v);
                        if (d2 < best2) {
                            best2 = d2; r.found = 1; r.isSphere = 0; r.objectIndex = k; r.triIndex = t; r.uv[0] = u; r.uv[1] = v;
                            bestP = rt_bary_point(a, b, c, u, v);
                        }
                    }
            }
            if (r.found) {
                r.dst = rt_sqrt(best2);
                if (r.isSphere) { r.triIndex = 0; r.uv[0] = r.uv[1] = 0.f; }
                r.point[0] = bestP.x; r.point[1] = bestP.y; r.point[2] = bestP.z;
            }
        }
        out[i] = r;
    }
    return 0;
}

}  // extern "C"
