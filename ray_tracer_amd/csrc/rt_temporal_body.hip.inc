// rt_temporal_body.hip.inc — the body of the temporal pass, included once per kernel by rt_kernels.hip.h with RT_TP_MOTION 0
// (k_tp_accumulate) and 1 (k_tp_accumulate_motion, which also has the motion table `mo`), so that the two cannot drift. It is text
// and not an inlined function on purpose: behind a function call, however inlined, the compiler commutes the operands of one
// multiply of k_tp_accumulate, and that kernel is to stay instruction for instruction what it was (DESIGN.md, "Moved objects
// and spheres"). In scope: f, cam, mats, materialCount, maxHistory, normalCos, depthTolerance.
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u), y = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
    if (x >= f.width || y >= f.height) return;
    const size_t n = (size_t)f.width * f.height, p = (size_t)y * f.width + x;
    const uint4 id = f.ids[p];
    const float4 c = f.rgba[p];
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!((id.w & 1u) && id.z < materialCount && rt_global(mats)[3 * id.z + 1].w == 0.f)) {   // kept: a miss or an emitter
        f.out[p] = c;
        f.moments[p] = zero;
        f.next[p] = zero; f.next[n + p] = zero; f.next[2 * n + p] = zero;
        return;
    }
    const float4 a = f.albedo[p], ndp = f.normalDepth[p], pos = f.position[p];
    const rt_vec3 d = rt_v3(rt_max(a.x, 1e-3f), rt_max(a.y, 1e-3f), rt_max(a.z, 1e-3f));
    const rt_vec3 e = rt_v3(c.x / d.x, c.y / d.y, c.z / d.z), np = f4xyz(ndp);
    const float l = (0.2126f * e.x + 0.7152f * e.y) + 0.0722f * e.z;
    const uint32_t keyObject = id.x, keyMaterial = (id.z << 1) | ((id.w >> 1) & 1u);
    rt_vec3 eh = e;
    float m1 = l, m2 = l * l, N = 1.f;
    rt_vec3 pp = f4xyz(pos), nn = np;   // P~, n~: what the previous camera and the tap tests see
#if RT_TP_MOTION
    if (f.prev && tp_previous_surface(mo, id, pos, np, pp, nn)) {
#else
    if (f.prev) {
#endif
        const rt_vec3 v = rt_sub(pp, rt_v3(cam.pos[0], cam.pos[1], cam.pos[2]));
        const float* m = cam.rot;   // q = M^T v: the inverse of primary_dir's rotation
        const rt_vec3 q = rt_v3((m[0] * v.x + m[1] * v.y) + m[2] * v.z, (m[4] * v.x + m[5] * v.y) + m[6] * v.z, (m[8] * v.x + m[9] * v.y) + m[10] * v.z);
        if (q.z > 0.f) {
            const float s = cam.bottomLeft[2] / q.z;
            const float fx = ((q.x * s - cam.bottomLeft[0]) / cam.planeWidth) * (float)f.width;
            const float fy = ((q.y * s - cam.bottomLeft[1]) / cam.planeHeight) * (float)f.height;
            // a tap can lie inside the image only for floor(fx) in [-1, width - 1]; the comparisons also turn away NaN and infinity
            if (fx >= -1.f && fx < (float)f.width && fy >= -1.f && fy < (float)f.height) {
                const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy), tx = fx - flx, ty = fy - fly;
                const int x0 = (int)flx, y0 = (int)fly;
                const float dist = rt_sqrt(rt_dot(v, v)), tol = depthTolerance * dist;
                float S = 0.f, sN = 0.f, s1 = 0.f, s2 = 0.f;
                rt_vec3 se = rt_v3(0.f, 0.f, 0.f);
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int qy = y0 + j;
                    if (qy < 0 || qy >= (int)f.height) continue;
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int qx = x0 + i;
                        if (qx < 0 || qx >= (int)f.width) continue;
                        const size_t t = (size_t)qy * f.width + (uint32_t)qx;
                        const float4 h0 = f.prev[t];
                        if (!(h0.w > 0.f)) continue;
                        const float4 h1 = f.prev[n + t], h2 = f.prev[2 * n + t];
                        if (__float_as_uint(h1.w) != keyObject || __float_as_uint(h2.w) != keyMaterial) continue;
                        if (!(rt_dot(nn, f4xyz(h2)) >= normalCos)) continue;
                        if (!(rt_abs(dist - h1.z) <= tol)) continue;
                        const float w = (i ? tx : 1.f - tx) * (j ? ty : 1.f - ty);
                        S += w;
                        se = rt_add(se, rt_scale(f4xyz(h0), w));
                        sN += w * h0.w; s1 += w * h1.x; s2 += w * h1.y;
                    }
                }
                if (S >= 1e-3f) {
                    const rt_vec3 he = rt_v3(se.x / S, se.y / S, se.z / S);
                    const float h1m = s1 / S, h2m = s2 / S;
                    N = rt_min(sN / S + 1.f, maxHistory);
                    const float k = 1.f / N;
                    eh = rt_add(he, rt_scale(rt_sub(e, he), k));
                    m1 = h1m + k * (l - h1m);
                    m2 = h2m + k * (l * l - h2m);
                }
            }
        }
    }
    f.out[p] = make_float4(eh.x * d.x, eh.y * d.y, eh.z * d.z, c.w);
    f.moments[p] = make_float4(m1, m2, rt_max(0.f, m2 - m1 * m1), N);
    f.next[p] = mk4(eh, N);
    f.next[n + p] = make_float4(m1, m2, ndp.w, __uint_as_float(keyObject));
    f.next[2 * n + p] = mk4(np, __uint_as_float(keyMaterial));
