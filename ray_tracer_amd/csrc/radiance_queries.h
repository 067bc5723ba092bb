// radiance_queries.h — the host logic of the radiance queries (rt_query_radiance and its _host form): what they refuse, in which
// order and with which words, the pieces a batch runs in, the bytes of its arrays and the frame's RNG seed. Nothing
// in this pair of files needs a device: it does pointer arithmetic only and never dereferences an array of a batch. rt_device.hip
// gathers the facts, asks here, and allocates, copies and launches; tests/radiance_queries_check.cpp pins every message and figure
// on the CPU, with made-up addresses. (ray_queries.h is the same for the hit queries; DESIGN.md, "Radiance queries")
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"

enum { RT_RADIANCE_MAX_SLOTS = 1 << 30 };          // a piece's rays live in path-state slots [0, piece): slot ids have 30 bits
enum { RT_RADIANCE_BOUNCE_LIMIT = (1 << 28) - 1 }; // the bounce index has 28 bits of att.w (rt_render refuses the same)

// What a radiance entry point (fn) refuses before anything is allocated or written, in this order: no uploaded scene; a NULL
// batch or NULL params; origins, dirs or the output NULL with n > 0; tmax not NULL; samples 0; bounceLimit >= 2^28 - 1;
// n >= 2^30. Empty: accepted (n == 0 is once there are a scene, a batch and params, whatever else they hold: the call does nothing).
std::string check_radiance_query(const char* fn, bool sceneUploaded, const RtRayBatch* rays, const RtRadianceParams* params, const void* out);

// A batch of n rays in consecutive pieces of at most maxSlots rays (rt_set_tuning("radiance_max_kslots") x 1024; at least one
// ray, at most 2^30 - 1): piece k holds rays [first, first + n) of the batch, in slots [0, n).
struct RadiancePiece { uint32_t first, n; };
uint32_t radiance_piece_cap(uint64_t maxSlots);                   // maxSlots clamped to 1 .. 2^30 - 1
uint32_t radiance_piece_count(uint32_t n, uint64_t maxSlots);     // 0 for n == 0
RadiancePiece radiance_piece(uint32_t n, uint64_t maxSlots, uint32_t k);

// The bytes of a batch's arrays (size_t: 2^30 - 1 results of 16 bytes are past 32 bits): origins and dirs 12 n each, the optional
// ids 4 n (0 when the batch has none), the result 16 n
struct RadianceShape { size_t vecBytes, idBytes, outBytes; };
RadianceShape radiance_shape(uint32_t n, bool hasIds);

// uint(random(frameCount) * 23892183) (raytrace.comp:561), as render_impl computes it for a frame
uint32_t radiance_starting_seed(uint32_t frameCount);
