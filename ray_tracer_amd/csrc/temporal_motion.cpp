// temporal_motion.cpp — the motion table of rt_temporal_accumulate, derived on the host (temporal_motion.h). Host only.

#include "temporal_motion.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

float4 flag_record(uint32_t flag) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    memcpy(&v.x, &flag, 4);
    return v;
}

void row(const float4& r, double out[4]) { out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w; }

}  // namespace

MotionTable motion_table(const PlacementSnapshot& prev, const PlacementSnapshot& now) {
    MotionTable t;
    const uint32_t nPrev = (uint32_t)prev.bvhIndex.size(), nNow = (uint32_t)now.bvhIndex.size();
    t.objectCount = nNow;
    t.objects.assign((size_t)std::max(nNow, 1u) * RT_MOTION_OBJECT_RECORDS, make_float4(0.f, 0.f, 0.f, 0.f));
    t.replacedObjects = std::max(nPrev, nNow) - std::min(nPrev, nNow);
    for (uint32_t o = 0; o < nNow; o++) {
        float4* rec = &t.objects[(size_t)o * RT_MOTION_OBJECT_RECORDS];
        if (o >= nPrev) { rec[0] = flag_record(RT_MOTION_REPLACED); continue; }
        if (prev.bvhIndex[o] != now.bvhIndex[o]) {
            rec[0] = flag_record(RT_MOTION_REPLACED);
            t.replacedObjects++;
            continue;
        }
        if (!memcmp(&prev.fwd[3 * (size_t)o], &now.fwd[3 * (size_t)o], 3 * sizeof(float4)) &&
            !memcmp(&prev.inv[3 * (size_t)o], &now.inv[3 * (size_t)o], 3 * sizeof(float4)))
            continue;   // bitwise equal: flag 0
        rec[0] = flag_record(RT_MOTION_MOVED);
        t.movedObjects++;
        double fp[3][4], ip[3][4], fn[3][4], in[3][4];
        for (int r = 0; r < 3; r++) {
            row(prev.fwd[3 * (size_t)o + r], fp[r]); row(prev.inv[3 * (size_t)o + r], ip[r]);
            row(now.fwd[3 * (size_t)o + r], fn[r]); row(now.inv[3 * (size_t)o + r], in[r]);
        }
        for (int i = 0; i < 3; i++) {
            double d[4], g[3];
            for (int j = 0; j < 4; j++) {
                d[j] = (fp[i][0] * in[0][j] + fp[i][1] * in[1][j]) + fp[i][2] * in[2][j];
                if (j == 3) d[j] += fp[i][3];   // the row (0, 0, 0, 1) both matrices end with
            }
            for (int j = 0; j < 3; j++) g[j] = (ip[0][i] * fn[j][0] + ip[1][i] * fn[j][1]) + ip[2][i] * fn[j][2];
            rec[1 + i] = make_float4((float)d[0], (float)d[1], (float)d[2], (float)d[3]);
            rec[4 + i] = make_float4((float)g[0], (float)g[1], (float)g[2], 0.f);
        }
    }
    const uint32_t sPrev = (uint32_t)prev.spheres.size(), sNow = (uint32_t)now.spheres.size();
    t.sphereCount = sNow;
    t.spheres.assign((size_t)std::max(sNow, 1u) * RT_MOTION_SPHERE_RECORDS, make_float4(0.f, 0.f, 0.f, 0.f));
    t.replacedSpheres = std::max(sPrev, sNow) - std::min(sPrev, sNow);
    for (uint32_t s = 0; s < sNow; s++) {
        float4* rec = &t.spheres[(size_t)s * RT_MOTION_SPHERE_RECORDS];
        uint32_t flag = RT_MOTION_UNMOVED;
        if (s >= sPrev) {
            flag = RT_MOTION_REPLACED;
        } else if (memcmp(&prev.spheres[s], &now.spheres[s], sizeof(float4))) {
            const float4 c = now.spheres[s], cp = prev.spheres[s];
            const float ratio = (float)((double)cp.w / (double)c.w);
            if (std::isfinite(ratio)) {
                flag = RT_MOTION_MOVED;
                t.movedSpheres++;
                rec[0] = make_float4(c.x, c.y, c.z, ratio);
                rec[1] = make_float4(cp.x, cp.y, cp.z, 0.f);
            } else {   // a sphere of radius 0 (or not a number) has no surface to follow
                flag = RT_MOTION_REPLACED;
                t.replacedSpheres++;
            }
        }
        memcpy(&rec[1].w, &flag, 4);
    }
    return t;
}
