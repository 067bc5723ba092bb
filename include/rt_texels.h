/*
 * rt_texels.h — the one rule of the lightmap texel passes (rt_bake_texels, rt_texels_exhaustive_host, rt_dilate_texels and their
 * host forms), compiled by the host and by the device from this text, under rt_det_math.h's discipline: RT_HD, no contraction
 * (-ffp-contract=off), no library math, a fixed evaluation order. ("Lightmap texels")
 *
 * The rule.
 *  - A map is W x H texels, each 1 .. 8192, rows top to bottom as textures are here. Texel (x, y) has its centre at
 *    u = (x + 0.5) / W, v = 1 - (y + 0.5) / H: the texel rt_tex_index(u, W), rt_tex_index(1 - v, H) picks, so a baked map uploaded
 *    as a texture lands where the sampler reads it.
 *  - Coverage is decided in exact integers on a grid of 256 sub-texels. A uv corner (u, v) (fp32, as triUV holds it) snaps to
 *    X = rint((double)u * (double)(256 W)), Y = rint((1 - (double)v) * (double)(256 H)), ties to even (rt_texel_rint: the
 *    2^52 trick, exact below 2^51). The centre of texel (x, y) is (256 x + 128, 256 y + 128).
 *  - A triangle is SKIPPED (covers nothing) when a uv component is not finite, when |X| or |Y| >= 2^27, or when its snapped doubled
 *    area A = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0) is 0 (two coincident uv corners, hit_uv's (0.5, 0.5) fallback, among them).
 *  - Either winding is accepted. With s = sign(A) the three edge functions at a centre C are
 *        E0 = s cross(P2 - P1, C - P1), E1 = s cross(P0 - P2, C - P2), E2 = s cross(P1 - P0, C - P0), E0 + E1 + E2 = |A|,
 *    cross(d, r) = d.x r.y - d.y r.x, so the inside is where all three are positive. A centre is covered when each Ek > 0, or
 *    Ek == 0 on a TOP or LEFT edge: with (dx, dy) = s x the edge's direction, a left edge has dy < 0 (E grows with x: the inside is
 *    to its right) and a top edge has dy == 0 and dx > 0 (E grows with Y, which runs downwards: the inside is below). The two
 *    triangles on a shared edge see it with opposite (dx, dy) once normalised, whatever their windings, so a centre on it belongs
 *    to exactly one; a centre on a shared vertex to at most one. Coordinates are below 2^27 and centres below 2^21 + 2^7, differences
 *    below 2^28, products below 2^56, edge values below 2^57.
 *  - The owner of a texel is the lowest triangle index among the object's triangles that cover its centre; `overlapped` when two
 *    or more do.
 *  - The record, from the owner's E1, E2 and |A|: u = (float)((double)E1 / (double)|A|), v = (float)((double)E2 / (double)|A|),
 *    w = (1 - u) - v (rt_texel_bary). point = rt_bary_point(a, b, c, u, v) of the world corners, placed as rt_query_nearest places
 *    them (the forward rows; an identity object's corners as they are). normal = rt_normalize(fwd x ((n0 w + n1 u) + n2 v)),
 *    reconstruct_hit's expression for a front-face hit without the bump map; always through the forward rows (DESIGN.md shows
 *    that reconstruct_hit's identity shortcut cannot change a bit of it). A normal that is not finite is replaced by the normalised
 *    world face normal cross(b - a, c - a), negated when its dot product with fwd x ((n0 + n1) + n2) is negative; if that is not
 *    finite either the texel is empty and counted as degenerate.
 *  - Dilation (rt_dilate_texel): pass k (from 1) reads the previous state; a texel with fill 0 and at least one 8-neighbour (no
 *    wrap) with fill != 0 gets the neighbours' rgb summed from +0 in the order (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1),
 *    (0,1), (1,1), divided by (float)count, alpha 0 and fill 1 + k; every other texel is copied.
 */
#ifndef RT_TEXELS_H
#define RT_TEXELS_H

#include "rt_point_query.h"

#define RT_TEXEL_SUB 256            /* sub-texels per texel */
#define RT_TEXEL_MAX_SIZE 8192u     /* width, height: 1 .. 8192 */
#define RT_TEXEL_BLOCK 8u           /* a work item of k_texel_cover: 8 x 8 texels, one per lane */
#define RT_TEXEL_EMPTY 0xffffffffu  /* the owner plane's "no triangle" */
#define RT_TEXEL_MAX_PASSES 254u    /* fill = 1 + pass fits a byte */

/* the three 4-float rows of a forward matrix: {m0, m4, m8, m12}, {m1, m5, m9, m13}, {m2, m6, m10, m14}; rt_xform_*'s sums */
typedef struct rt_rows { float r[3][4]; } rt_rows;
RT_HD rt_rows rt_rows_of(const float* m) {
    rt_rows f;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) f.r[i][j] = m[j * 4 + i];
    return f;
}
RT_HD rt_vec3 rt_rows_dir(const rt_rows* f, rt_vec3 v) {
    return rt_v3((f->r[0][0] * v.x + f->r[0][1] * v.y) + f->r[0][2] * v.z, (f->r[1][0] * v.x + f->r[1][1] * v.y) + f->r[1][2] * v.z,
                 (f->r[2][0] * v.x + f->r[2][1] * v.y) + f->r[2][2] * v.z);
}
RT_HD rt_vec3 rt_rows_point(const rt_rows* f, rt_vec3 v) {
    return rt_v3(((f->r[0][0] * v.x + f->r[0][1] * v.y) + f->r[0][2] * v.z) + f->r[0][3],
                 ((f->r[1][0] * v.x + f->r[1][1] * v.y) + f->r[1][2] * v.z) + f->r[1][3],
                 ((f->r[2][0] * v.x + f->r[2][1] * v.y) + f->r[2][2] * v.z) + f->r[2][3]);
}

RT_HD bool rt_texel_finite(float x) { return !rt_isnan(x) && !rt_isinf(x); }
RT_HD bool rt_texel_finite3(rt_vec3 v) { return rt_texel_finite(v.x) && rt_texel_finite(v.y) && rt_texel_finite(v.z); }

/* round to the nearest integer, ties to even, for |p| < 2^51: the sum with 2^52 has no fraction bits left (no contraction, no
 * reassociation: the sum is rounded to a double before the difference) */
RT_HD int64_t rt_texel_rint(double p) {
    const double big = 4503599627370496.0; /* 2^52 */
    const double t = (p < 0.0 ? -p : p) + big;
    const double r = t - big;
    return p < 0.0 ? -(int64_t)r : (int64_t)r;
}

/* one uv component on the sub-texel grid of a map axis of `size` texels (flip: the v axis, rows run downwards).
 * false: not finite, or |result| >= 2^27 */
RT_HD bool rt_texel_snap(float c, bool flip, uint32_t size, int64_t* out) {
    if (!rt_texel_finite(c)) return false;
    const double p = (flip ? 1.0 - (double)c : (double)c) * (double)((uint32_t)RT_TEXEL_SUB * size);
    if (!(p > -134217729.0 && p < 134217729.0)) return false;
    const int64_t v = rt_texel_rint(p);
    if (v >= 134217728ll || v <= -134217728ll) return false;
    *out = v;
    return true;
}

/* A triangle's snapped uv corners, normalised: sign = +1 / -1 is the sign of the doubled area, area its magnitude (> 0) */
typedef struct rt_texel_tri {
    int64_t x0, y0, x1, y1, x2, y2;
    int64_t area, sign;
} rt_texel_tri;

/* uv: {u0 v0 u1 v1 u2 v2}. false: the triangle is skipped */
RT_HD bool rt_texel_setup(const float* uv, uint32_t width, uint32_t height, rt_texel_tri* t) {
    if (!rt_texel_snap(uv[0], false, width, &t->x0) || !rt_texel_snap(uv[1], true, height, &t->y0)) return false;
    if (!rt_texel_snap(uv[2], false, width, &t->x1) || !rt_texel_snap(uv[3], true, height, &t->y1)) return false;
    if (!rt_texel_snap(uv[4], false, width, &t->x2) || !rt_texel_snap(uv[5], true, height, &t->y2)) return false;
    const int64_t a = (t->x1 - t->x0) * (t->y2 - t->y0) - (t->x2 - t->x0) * (t->y1 - t->y0);
    if (a == 0) return false;
    t->sign = a > 0 ? 1 : -1;
    t->area = a > 0 ? a : -a;
    return true;
}

/* the normalised value at (cx, cy) of the edge from (ax, ay) to (bx, by), and whether a value of 0 on it counts (top or left) */
RT_HD int64_t rt_texel_edge_value(int64_t sign, int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t cx, int64_t cy) {
    return sign * ((bx - ax) * (cy - ay) - (by - ay) * (cx - ax));
}
RT_HD bool rt_texel_edge_is_closed(int64_t sign, int64_t ax, int64_t ay, int64_t bx, int64_t by) {
    const int64_t dx = sign * (bx - ax), dy = sign * (by - ay);
    return dy < 0 || (dy == 0 && dx > 0);
}
/* edge k lies opposite corner k: edge 0 runs from corner 1 to corner 2, edge 1 from 2 to 0, edge 2 from 0 to 1 */
RT_HD int64_t rt_texel_edge(const rt_texel_tri* t, int k, int64_t cx, int64_t cy) {
    return k == 0 ? rt_texel_edge_value(t->sign, t->x1, t->y1, t->x2, t->y2, cx, cy)
         : k == 1 ? rt_texel_edge_value(t->sign, t->x2, t->y2, t->x0, t->y0, cx, cy)
                  : rt_texel_edge_value(t->sign, t->x0, t->y0, t->x1, t->y1, cx, cy);
}
RT_HD bool rt_texel_edge_closed(const rt_texel_tri* t, int k) {
    return k == 0 ? rt_texel_edge_is_closed(t->sign, t->x1, t->y1, t->x2, t->y2)
         : k == 1 ? rt_texel_edge_is_closed(t->sign, t->x2, t->y2, t->x0, t->y0)
                  : rt_texel_edge_is_closed(t->sign, t->x0, t->y0, t->x1, t->y1);
}
RT_HD int64_t rt_texel_centre(uint32_t i) { return (int64_t)i * RT_TEXEL_SUB + RT_TEXEL_SUB / 2; }

/* whether the centre of texel (x, y) is covered; e1, e2 (either may be NULL): the edge values the record is made from */
RT_HD bool rt_texel_covers(const rt_texel_tri* t, uint32_t x, uint32_t y, int64_t* e1, int64_t* e2) {
    const int64_t cx = rt_texel_centre(x), cy = rt_texel_centre(y);
    const int64_t v0 = rt_texel_edge(t, 0, cx, cy), v1 = rt_texel_edge(t, 1, cx, cy), v2 = rt_texel_edge(t, 2, cx, cy);
    if (e1) *e1 = v1;
    if (e2) *e2 = v2;
    return (v0 > 0 || (v0 == 0 && rt_texel_edge_closed(t, 0))) && (v1 > 0 || (v1 == 0 && rt_texel_edge_closed(t, 1))) &&
           (v2 > 0 || (v2 == 0 && rt_texel_edge_closed(t, 2)));
}

/* floor(v / 256) for either sign */
RT_HD int64_t rt_texel_floor_sub(int64_t v) { return v >= 0 ? v / RT_TEXEL_SUB : -((-v + (RT_TEXEL_SUB - 1)) / RT_TEXEL_SUB); }

/* The texels whose centres lie in the triangle's bounding box, clipped to the map: [x0, x1] x [y0, y1]. false: none */
typedef struct rt_texel_box { uint32_t x0, y0, x1, y1; } rt_texel_box;
RT_HD bool rt_texel_bounds(const rt_texel_tri* t, uint32_t width, uint32_t height, rt_texel_box* b) {
    int64_t lox = t->x0 < t->x1 ? t->x0 : t->x1, hix = t->x0 > t->x1 ? t->x0 : t->x1;
    int64_t loy = t->y0 < t->y1 ? t->y0 : t->y1, hiy = t->y0 > t->y1 ? t->y0 : t->y1;
    lox = t->x2 < lox ? t->x2 : lox; hix = t->x2 > hix ? t->x2 : hix;
    loy = t->y2 < loy ? t->y2 : loy; hiy = t->y2 > hiy ? t->y2 : hiy;
    /* centres 256 i + 128 in [lo, hi]: i from ceil((lo - 128) / 256) to floor((hi - 128) / 256) */
    int64_t x0 = rt_texel_floor_sub(lox - RT_TEXEL_SUB / 2 + (RT_TEXEL_SUB - 1)), x1 = rt_texel_floor_sub(hix - RT_TEXEL_SUB / 2);
    int64_t y0 = rt_texel_floor_sub(loy - RT_TEXEL_SUB / 2 + (RT_TEXEL_SUB - 1)), y1 = rt_texel_floor_sub(hiy - RT_TEXEL_SUB / 2);
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > (int64_t)width - 1) x1 = (int64_t)width - 1;
    if (y1 > (int64_t)height - 1) y1 = (int64_t)height - 1;
    if (x0 > x1 || y0 > y1) return false;
    b->x0 = (uint32_t)x0; b->y0 = (uint32_t)y0; b->x1 = (uint32_t)x1; b->y1 = (uint32_t)y1;
    return true;
}
/* the 8 x 8 blocks the box touches: columns x0 / 8 .. x1 / 8, rows likewise; at most 1024 x 1024 */
RT_HD uint32_t rt_texel_box_blocks(const rt_texel_box* b) {
    return (b->x1 / RT_TEXEL_BLOCK - b->x0 / RT_TEXEL_BLOCK + 1u) * (b->y1 / RT_TEXEL_BLOCK - b->y0 / RT_TEXEL_BLOCK + 1u);
}
/* block k of the box, row-major over its block columns: the texel of its top-left corner */
RT_HD void rt_texel_box_block(const rt_texel_box* b, uint32_t k, uint32_t* x, uint32_t* y) {
    const uint32_t cols = b->x1 / RT_TEXEL_BLOCK - b->x0 / RT_TEXEL_BLOCK + 1u;
    *x = (b->x0 / RT_TEXEL_BLOCK + k % cols) * RT_TEXEL_BLOCK;
    *y = (b->y0 / RT_TEXEL_BLOCK + k / cols) * RT_TEXEL_BLOCK;
}
/* how many work items a triangle is: 0 when it is skipped or its box holds no centre */
RT_HD uint32_t rt_texel_tri_blocks(const float* uv, uint32_t width, uint32_t height, bool* skipped) {
    rt_texel_tri t;
    rt_texel_box b;
    *skipped = !rt_texel_setup(uv, width, height, &t);
    if (*skipped || !rt_texel_bounds(&t, width, height, &b)) return 0u;
    return rt_texel_box_blocks(&b);
}
/* whether the block of 8 x 8 texels at (bx, by) lies wholly outside one edge: the edge's value is negative at the centres of the
 * block's four corner texels (an edge function is linear, so it is negative on every centre between them) */
RT_HD bool rt_texel_block_outside(const rt_texel_tri* t, uint32_t bx, uint32_t by) {
    const int64_t x0 = rt_texel_centre(bx), x1 = rt_texel_centre(bx + RT_TEXEL_BLOCK - 1u), y0 = rt_texel_centre(by), y1 = rt_texel_centre(by + RT_TEXEL_BLOCK - 1u);
    if (rt_texel_edge(t, 0, x0, y0) < 0 && rt_texel_edge(t, 0, x1, y0) < 0 && rt_texel_edge(t, 0, x0, y1) < 0 && rt_texel_edge(t, 0, x1, y1) < 0) return true;
    if (rt_texel_edge(t, 1, x0, y0) < 0 && rt_texel_edge(t, 1, x1, y0) < 0 && rt_texel_edge(t, 1, x0, y1) < 0 && rt_texel_edge(t, 1, x1, y1) < 0) return true;
    if (rt_texel_edge(t, 2, x0, y0) < 0 && rt_texel_edge(t, 2, x1, y0) < 0 && rt_texel_edge(t, 2, x0, y1) < 0 && rt_texel_edge(t, 2, x1, y1) < 0) return true;
    return false;
}

/* the barycentrics of a covered centre from its edge values and the area */
RT_HD void rt_texel_bary(int64_t e1, int64_t e2, int64_t area, float* u, float* v, float* w) {
    *u = (float)((double)e1 / (double)area);
    *v = (float)((double)e2 / (double)area);
    *w = (1.f - *u) - *v;
}

/* What a covered texel's record holds. a, b, c: the object-space corners; n0, n1, n2: the vertex normals; fwd: the object's forward
 * rows; identity: RT_OBJ_FWD_IDENTITY (the corners are used as they are). false: a degenerate texel (no finite normal) */
typedef struct rt_texel_record { rt_vec3 point, normal; float u, v; } rt_texel_record;
RT_HD bool rt_texel_make_record(int64_t e1, int64_t e2, int64_t area, rt_vec3 a, rt_vec3 b, rt_vec3 c, rt_vec3 n0, rt_vec3 n1, rt_vec3 n2,
                                const rt_rows* fwd, bool identity, rt_texel_record* r) {
    float u, v, w;
    rt_texel_bary(e1, e2, area, &u, &v, &w);
    if (!identity) { a = rt_rows_point(fwd, a); b = rt_rows_point(fwd, b); c = rt_rows_point(fwd, c); }
    r->u = u; r->v = v;
    r->point = rt_bary_point(a, b, c, u, v);
    const rt_vec3 ni = rt_add(rt_add(rt_scale(n0, w), rt_scale(n1, u)), rt_scale(n2, v));
    rt_vec3 n = rt_normalize(rt_rows_dir(fwd, ni));
    if (!rt_texel_finite3(n)) {
        rt_vec3 face = rt_cross(rt_sub(b, a), rt_sub(c, a));
        const rt_vec3 sum = rt_rows_dir(fwd, rt_add(rt_add(n0, n1), n2));
        if (rt_dot(face, sum) < 0.f) face = rt_neg(face);
        n = rt_normalize(face);
        if (!rt_texel_finite3(n)) return false;
    }
    r->normal = n;
    return true;
}

/* One texel of one dilation pass (pass k counted from 1): reads the previous planes, writes out[4] and *fillOut */
RT_HD void rt_dilate_texel(uint32_t width, uint32_t height, uint32_t x, uint32_t y, uint32_t pass, const float* rgba, const uint8_t* fill,
                           float* out, uint8_t* fillOut) {
    const size_t i = (size_t)y * width + x;
    if (fill[i] != 0) {
        out[0] = rgba[4 * i]; out[1] = rgba[4 * i + 1]; out[2] = rgba[4 * i + 2]; out[3] = rgba[4 * i + 3];
        *fillOut = fill[i];
        return;
    }
    float r = 0.f, g = 0.f, b = 0.f;
    uint32_t count = 0;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            if (dx == 0 && dy == 0) continue;
            const int64_t nx = (int64_t)x + dx, ny = (int64_t)y + dy;
            if (nx < 0 || ny < 0 || nx >= (int64_t)width || ny >= (int64_t)height) continue;
            const size_t j = (size_t)ny * width + (size_t)nx;
            if (fill[j] == 0) continue;
            r = r + rgba[4 * j]; g = g + rgba[4 * j + 1]; b = b + rgba[4 * j + 2];
            count++;
        }
    if (count == 0) {
        out[0] = rgba[4 * i]; out[1] = rgba[4 * i + 1]; out[2] = rgba[4 * i + 2]; out[3] = rgba[4 * i + 3];
        *fillOut = 0;
        return;
    }
    const float n = (float)count;
    out[0] = r / n; out[1] = g / n; out[2] = b / n; out[3] = 0.f;
    *fillOut = (uint8_t)(1u + pass);
}

#endif /* RT_TEXELS_H */
