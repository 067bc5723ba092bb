// irradiance_queries.h — the host logic of the baked-light queries (rt_query_irradiance, rt_query_sh_probes and their _host forms):
// what they refuse, in which order and with which words, the chunks of whole points a batch runs in, the bytes of its arrays and
// of the ctx scratch a chunk's rays live in, and the host forms of the rule (rt_irradiance_rays_host, rt_irradiance_gather_host;
// include/rt_irradiance.h). Nothing in this pair of files needs a device, and the checks and the arithmetic never dereference an
// array of a batch. rt_device.hip gathers the facts, asks here, and allocates, copies and launches; tests/irradiance_check.cpp
// pins every message and figure on the CPU, with made-up addresses. (radiance_queries.h is the same for the radiance queries;
// DESIGN.md, "Irradiance and SH probes")
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"

enum { RT_IRRADIANCE_MAX_POINTS = 1 << 30 };   // n < 2^30, as every batch query

// What an entry point (fn; sphere: the probe form, which reads no normals) refuses before anything is allocated or written, in
// this order: no uploaded scene; a NULL batch or NULL params; points, normals (irradiance form) or the output NULL with n > 0;
// samples 0 or >= 2^24; bounceLimit >= 2^28 - 1; bias not finite or < 0; samples > the piece cap (radiance_piece_cap(maxSlots):
// one point's rays must fit one radiance piece); n >= 2^30. Empty: accepted (n == 0 is once there are a scene, a batch and params).
std::string check_irradiance_query(const char* fn, bool sphere, bool sceneUploaded, const RtPointNormalBatch* batch,
                                   const RtIrradianceParams* params, const void* out, uint64_t maxSlots);

// A batch of n points of S samples each in consecutive chunks of whole points, as many as keep chunk x S <= the piece cap, so that
// each chunk's rays are one radiance piece: chunk k holds points [first, first + n) of the batch.
struct IrradianceChunk { uint32_t first, n; };
uint32_t irradiance_chunk_points(uint32_t samples, uint64_t maxSlots);                // cap / S; 0 when S is 0 or above the cap
uint32_t irradiance_chunk_count(uint32_t n, uint32_t samples, uint64_t maxSlots);     // 0 for n == 0 or no points per chunk
IrradianceChunk irradiance_chunk(uint32_t n, uint32_t samples, uint64_t maxSlots, uint32_t k);

// The bytes of a batch's arrays: points and normals 12 n each, the optional ids 4 n, the result 16 n (irradiance) or 108 n (probes)
struct IrradianceShape { size_t vecBytes, idBytes, outBytes; };
IrradianceShape irradiance_shape(uint32_t n, bool hasIds, bool sphere);

// The ctx scratch of a chunk of `rays` rays (at most the piece cap): the radiance records first (16-byte aligned), then the origins,
// the dirs (RtRayBatch's packed layout) and the ray ids: 44 bytes per ray
struct IrradianceScratch { size_t radiance, origins, dirs, ids, bytes; };
IrradianceScratch irradiance_scratch(uint32_t rays);
