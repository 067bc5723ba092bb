// rt_aov_record.hip.inc — one ray's hit record as the AOV planes hold it, included by rt_kernels.hip.h in k_aov_resolve
// (RT_AOV_MIRROR 0) and in k_guide_follow (RT_AOV_MIRROR 1: also `mirror`, whether shade_path<true> would reflect the ray at this
// hit), so that the two cannot drift. Text and not an inlined function, as rt_temporal_body.hip.inc is: behind a function the
// compiler allocates k_aov_resolve's registers differently, and that kernel is to stay instruction for instruction what it was.
// In scope: sc, ro, rd, hm (the traversal's record of the ray). Declares obj, tri, normalDepth, position, albedo, ids.
    const uint32_t obj = __float_as_uint(hm.y), tri = __float_as_uint(hm.z);
    float4 normalDepth = make_float4(0.f, 0.f, 0.f, hm.x), position = make_float4(0.f, 0.f, 0.f, 0.f), albedo = position;
    uint4 ids = make_uint4(RT_HIT_NONE, RT_HIT_NONE, RT_HIT_NONE, 0u);
#if RT_AOV_MIRROR
    bool mirror = false;
#endif
    if (obj != RT_HIT_NONE) {
        const bool sphere = (obj & RT_HIT_SPHERE) != 0u;
        const FullHit f = reconstruct_hit<true>(sc, ro, rd, obj, tri);
        const float4* mp = rt_global(sc.mats) + 3 * f.materialIndex;
        const float4 mA = mp[0];
        rt_vec3 a = rt_v3(mA.x, mA.y, mA.z);
        const uint32_t texSlot = __float_as_uint(mp[2].y);   // albedoIndex; 0xffffffff (-1) = none
        if (texSlot < sc.texCount && !sphere) a = rt_mul(a, albedo_texel(sc, texSlot, tri, obj, ro, rd));
#if RT_AOV_MIRROR
        // reflectance != 0 (raytrace.comp:466), the reflectance being the metalness texel where an uploaded map binds (shade_path<true>)
        float reflectance = mA.w;
        const uint32_t metalSlot = __float_as_uint(mp[2].z);   // metalnessIndex; 0xffffffff (-1) = none
        if (metalSlot < sc.texCount && !sphere)
            reflectance = rt_srgb8_to_linear(map_red8(sc, metalSlot, ((rt_global(sc.objMeta)[obj].w >> RT_OBJ_SAMPLER_SHIFT) & RT_OBJ_SAMPLER_MASK) == 1u, f.u, f.v, false, false));
        mirror = reflectance != 0.f;
#endif
        normalDepth = mk4(f.normal, hm.x);
        position = mk4(f.hitPoint, 1.f);
        albedo = mk4(a, 1.f);
        ids = make_uint4(obj & ~RT_HIT_SPHERE, sphere ? 0u : tri, f.materialIndex, 1u | (sphere ? 2u : 0u) | (f.frontFace ? 4u : 0u));
    }
