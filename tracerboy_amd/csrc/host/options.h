/* options.h -- every option tb_set_option accepts, once: its name, its default and what tb_set_option checks.  Reads go through
 * Options::get<OPT_name>() (context_internal.h: opt<OPT_name>(c)), which takes no default: a name that is not a row does not compile. */
#pragma once
#include <stdint.h>
#include <string.h>

namespace tbhost {

enum : uint32_t {
    OPT_NO_DEFAULT = 1u,     /* the default is not a constant (the kind of scene, ConvertOptions): read with ifSet, the call site has the fallback */
    OPT_RESETS_HISTORY = 2u, /* setting it invalidates the accumulated frames */
    OPT_NOT_NEGATIVE = 4u, OPT_ZERO_OR_ONE = 8u, /* the values tb_set_option accepts */
};

/* X(name, default, flags) */
#define TB_OPTIONS(X) \
    X(pipeline, 0, 0) X(frame_group, 0, 0) X(high_occupancy, 1, 0) X(stack_lds_cap, 0, 0) X(stack_overflow_max, 24, 0) X(node_layout, 0, 0) \
    X(primary_prepass, 1, 0) X(first_bounce, 0, 0) X(compact_hits, 1, 0) X(compact_stamp_bits, 32, 0) X(overlap_launches, 1, 0) \
    X(guided_groups, 1, 0) X(costly_first, 1, 0) X(costly_late_samples, 1ll << 40, 0) X(banded_items, 0, 0) X(camera_constants, 1, 0) \
    X(count_rays, 0, OPT_RESETS_HISTORY) X(aov, 0, OPT_RESETS_HISTORY) X(force_full_variant, 0, 0) X(debug_profile_groups, 0, 0) X(alpha_test, 0, 0) \
    X(debug_light_count, 0, OPT_RESETS_HISTORY | OPT_NOT_NEGATIVE) /* not 0: a call's TbPerFrameConstants::LightCount, whatever the scene holds (tests) */ \
    X(post_denoised, 0, 0) /* tb_post_process(LIT) reads the denoised still of tb_denoise */ \
    X(denoise_guides, 0, 0) /* tb_denoise: 0 = the last frame's AOVs, 1 = the guide pass's normals and positions, 2 = 1 + albedo demodulation */ \
    X(sr_conv_form, 1, OPT_ZERO_OR_ONE) /* the convolutions of the super-resolution network: 0 = plain, 1 = staged in LDS (the same bits, half the time) */ \
    X(adaptive, 0, 0) X(adaptive_min_frames, 1024 /* the reference's */, OPT_NOT_NEGATIVE) X(adaptive_test, 0, OPT_ZERO_OR_ONE) \
    X(wavefront_paths, 16ll << 20, 0) X(wavefront_grid, 256 * 8, 0) X(wavefront_segment, 4096, 0) X(wavefront_sort, 0, 0) X(wavefront_refill, 0, 0) \
    X(pooled_paths, 2, 0) X(pooled_samples, 256ll << 20, 0) X(pooled_profile, 0, 0) \
    X(split_trav, 4, 0) X(split_shade, 0, 0) X(split_ready, 32, 0) X(split_refill, 16, 0) X(split_wi, 85, 0) X(split_wl, 160, 0) \
    X(split_frame_group, 8, 0) X(split_stack_cap, 0, 0) X(split_spin_limit, 1 << 21, 0) X(split_profile, 0, 0) X(split_trav_last, 0, 0) \
    X(split_shade_prio, 0, 0) \
    X(bvh_builder, 0, 0) X(reinsertion_passes, -1, 0) X(reinsertion_share, 100, 0) X(presplit, 0, 0) X(wave_tree, -1, 0) X(wave_tree_threads, 0, OPT_NOT_NEGATIVE) X(node_order, 2, 0) \
    X(node_order_top_levels, 10, 0) X(scene_in_lds, 1, 0) X(lds_scene_budget, 40 * 1024, 0) \
    X(park_min, 0, OPT_NO_DEFAULT) X(flatten_instances, 0, OPT_NO_DEFAULT) X(flip_texture_uvs, 0, OPT_NO_DEFAULT) X(texture_use_hint, 0, OPT_NO_DEFAULT)

enum Opt {
#define X(name, def, flags) OPT_##name,
    TB_OPTIONS(X)
#undef X
    OPT_COUNT
};
struct OptionRow { const char* name; int64_t def; uint32_t flags; };
constexpr OptionRow kOptions[OPT_COUNT] = {
#define X(name, def, flags) {#name, def, flags},
    TB_OPTIONS(X)
#undef X
};
constexpr int64_t OptionDefault(Opt k) { return kOptions[k].def; }
inline int FindOption(const char* name) { for (int k = 0; k < OPT_COUNT; k++) if (!strcmp(kOptions[k].name, name)) return k; return -1; }

/* the values of a context; plain data, so that a device group hands them to its peers by assignment */
struct Options {
    int64_t value[OPT_COUNT] = {}; bool isSet[OPT_COUNT] = {};
    template <Opt K> int64_t get() const
    {
        static_assert(!(kOptions[K].flags & OPT_NO_DEFAULT), "this option has no constant default: ifSet<>() and the call site's fallback");
        return isSet[K] ? value[K] : kOptions[K].def;
    }
    template <Opt K> const int64_t* ifSet() const
    {
        static_assert((kOptions[K].flags & OPT_NO_DEFAULT) != 0, "this option has a default: get<>()");
        return isSet[K] ? &value[K] : nullptr;
    }
};

} // namespace tbhost
