/* pt_copies.h -- the lock-step kernel copies, described once: what each pt_variant_*.hip compiles, which of its kernels a launch may run
 * (pt_pick_form, a pure function), and the -D overrides of the experiment scripts.  Included by the kernel units (pt_variant.inc turns the unit's
 * row into its kernels and its launcher), by the host (context.cpp builds kVariants from the rows) and by tests/forms/forms_driver.cpp, which walks
 * the picker on the CPU: no HIP in here, plain C++17.
 *
 * Experiment overrides (every one spelled here and nowhere else, unless the kernel bodies read it):
 *   -DTB_MATTE_WAVES / TB_MATTE_LDS_WAVES / TB_ENV_WAVES / TB_SSS_WAVES / TB_VOL_WAVES / TB_SURF_WAVES=n   waves per SIMD of matte5 / matte6 /
 *       env5 / sss4 / vol4 / surf (scripts/ab_flags.sh, ab_device_flags.sh, build_sss_sweep.py, sss_waves_timing.sh); kernels and host read the row
 *   -DTB_ENV_STASH / TB_SSS_STASH / TB_VOL_STASH=n   LDS entries per lane the frame-group kernels of env5 / sss4 / vol4 keep behind the stacks
 *   -DTB_NO_OCCUPANCY_BOUND    measurement only (scripts/spill_share.sh): surf, sss4 and vol4 with all the registers they want, i.e. without spills
 *   -DTB_EXP_PROFILE_GROUPS    (scripts/c2_instruction_mix.py) the plain frame-group launch runs the kernel with the wave-occupancy profile of the
 *       counting copies compiled in -- trips per phase of the very launch shape bench.py times (host option debug_profile_groups hands it tg->rayStats)
 *   -DTB_WG_TIMELINE (pt_persistent.inc) and -DTB_EXP_DOUBLE=k (pt_device.hpp) are read by the kernel bodies alone. */
#pragma once
#include <stdint.h>
#include "pt_device_features.h"

#ifndef TB_MATTE_WAVES
#define TB_MATTE_WAVES 5
#endif
#ifndef TB_MATTE_LDS_WAVES
#define TB_MATTE_LDS_WAVES 6
#endif
#ifndef TB_ENV_WAVES
#define TB_ENV_WAVES 6
#endif
#ifndef TB_SURF_WAVES
#define TB_SURF_WAVES 4
#endif
#ifndef TB_SSS_WAVES
#define TB_SSS_WAVES 6
#endif
#ifndef TB_VOL_WAVES
#define TB_VOL_WAVES 4
#endif
#ifndef TB_ENV_STASH
#define TB_ENV_STASH 7
#endif
#ifndef TB_SSS_STASH
#define TB_SSS_STASH 0
#endif
#ifndef TB_VOL_STASH
#define TB_VOL_STASH 0
#endif
#ifdef TB_NO_OCCUPANCY_BOUND
#define PT_LIFTABLE(waves) 0 /* amdgpu_waves_per_eu(0) is no bound */
#else
#define PT_LIFTABLE(waves) waves
#endif
#ifdef TB_EXP_PROFILE_GROUPS
#define PT_PROFILE_GROUPS true
#else
#define PT_PROFILE_GROUPS false
#endif

#define PT_FEATS_SURF (PT_FEAT_ENV | PT_FEAT_SPECULAR | PT_FEAT_TEXTURES)
#define PT_FEATS_SSS (PT_FEATS_SURF | PT_FEAT_SSS)
#define PT_FEATS_VOL (PT_FEATS_SSS | PT_FEAT_MIX)

/* role of a copy within its feature set.  BASE: every form but the tuned ones (one pixel per lane, streaming, frame groups with the whole stack in
 * LDS) and the wavefront / pooled kernels of the set.  OCCUPANCY: the same feature set held to more waves per SIMD (fewer VGPRs, more scratch),
 * lock-step only -- the tuned frame-group kernels live here: split stack, layout C, the two-level walk, the pre-pass.  LDS_GROUPS: the frame-group
 * kernels of one-level scenes in LDS with the whole stack in LDS, nothing else. */
#define PT_ROLE_BASE 0
#define PT_ROLE_OCCUPANCY 1
#define PT_ROLE_LDS_GROUPS 2

/* One row per copy; the preprocessor reads the fields too (PT_FIELD), so they are literals:
 *   (name, feature set, feature bits, role, waves per SIMD, bound of the kernels' amdgpu_waves_per_eu, stash entries per lane,
 *    builds the counting kernels, builds the streaming kernel (pt_stream), a base copy that carries the pre-pass)
 * Why each occupancy was chosen is recorded in the copy's unit, with the measurements. */
#define PT_ROW_matte  (matte,  matte, 0u,            PT_ROLE_BASE,       4,                  4,                          0,            0, 1, 0)
#define PT_ROW_matte5 (matte5, matte, 0u,            PT_ROLE_OCCUPANCY,  TB_MATTE_WAVES,     TB_MATTE_WAVES,             0,            0, 0, 0)
#define PT_ROW_matte6 (matte6, matte, 0u,            PT_ROLE_LDS_GROUPS, TB_MATTE_LDS_WAVES, TB_MATTE_LDS_WAVES,         0,            0, 0, 0)
#define PT_ROW_env    (env,    env,   PT_FEAT_ENV,   PT_ROLE_BASE,       4,                  4,                          0,            0, 1, 0)
#define PT_ROW_env5   (env5,   env,   PT_FEAT_ENV,   PT_ROLE_OCCUPANCY,  TB_ENV_WAVES,       TB_ENV_WAVES,               TB_ENV_STASH, 0, 0, 0)
#define PT_ROW_surf   (surf,   surf,  PT_FEATS_SURF, PT_ROLE_BASE,       TB_SURF_WAVES,      PT_LIFTABLE(TB_SURF_WAVES), 0,            0, 1, 1)
#define PT_ROW_sss    (sss,    sss,   PT_FEATS_SSS,  PT_ROLE_BASE,       3,                  3,                          0,            0, 1, 0)
#define PT_ROW_sss4   (sss4,   sss,   PT_FEATS_SSS,  PT_ROLE_OCCUPANCY,  TB_SSS_WAVES,       PT_LIFTABLE(TB_SSS_WAVES),  TB_SSS_STASH, 0, 0, 0)
#define PT_ROW_vol    (vol,    vol,   PT_FEATS_VOL,  PT_ROLE_BASE,       3,                  3,                          0,            0, 1, 0)
#define PT_ROW_vol4   (vol4,   vol,   PT_FEATS_VOL,  PT_ROLE_OCCUPANCY,  TB_VOL_WAVES,       PT_LIFTABLE(TB_VOL_WAVES),  TB_VOL_STASH, 0, 0, 0)
#define PT_ROW_full   (full,   full,  PT_FEAT_ALL,   PT_ROLE_BASE,       3,                  3,                          0,            1, 1, 0)
#define PT_COPY_LIST(X) X(matte) X(matte5) X(matte6) X(env) X(env5) X(surf) X(sss) X(sss4) X(vol) X(vol4) X(full)

#define PT_CAT2(a, b) a##b
#define PT_CAT(a, b) PT_CAT2(a, b)
#define PT_FIELD2(field, row) field row
#define PT_FIELD(field, copy) PT_FIELD2(field, PT_CAT(PT_ROW_, copy)) /* e.g. PT_FIELD(PT_F_STASH, env5), usable in #if */
#define PT_F_FEATURES(name, set, features, role, waves, bound, stash, counting, streaming, prepass) (features)
#define PT_F_ROLE(name, set, features, role, waves, bound, stash, counting, streaming, prepass) role
#define PT_F_BOUND(name, set, features, role, waves, bound, stash, counting, streaming, prepass) bound
#define PT_F_STASH(name, set, features, role, waves, bound, stash, counting, streaming, prepass) stash
#define PT_F_STREAMING(name, set, features, role, waves, bound, stash, counting, streaming, prepass) streaming
#define PT_F_INIT(name, set, features, role, waves, bound, stash, counting, streaming, prepass) \
    {#name, #set, features, role, waves, stash, counting != 0, streaming != 0, prepass != 0}

struct PtCopy {
    const char* name; const char* set; uint32_t features; int role; uint32_t waves, stash; bool counting, streaming, prepassInBase;
    constexpr bool ext() const { return (features & PT_FEAT_EXT) != 0; } /* the full feature set: its kernels walk two levels in all their forms */
    constexpr bool prepass() const { return (role == PT_ROLE_OCCUPANCY || prepassInBase) && !ext(); } /* pt_primary / pt_first and the forms they feed */
};
#define PT_COPY_ROW(copy) PT_FIELD(PT_F_INIT, copy),
constexpr PtCopy kPtCopies[] = { PT_COPY_LIST(PT_COPY_ROW) };
constexpr int kNumPtCopies = (int)(sizeof(kPtCopies) / sizeof(kPtCopies[0]));

/* how a launcher (pt_launch_persistent_<copy>, pt_launch.h) is asked to run */
enum PtMode { PT_MODE_LOCKSTEP = 0,  /* one pixel per lane, or frame groups where TbDeviceTargets::samples is set */
              PT_MODE_STREAM,        /* pt_stream (option pipeline = 1) */
              PT_MODE_LIVE_GROUPS,   /* the frame-group kernels over TbDeviceTargets::liveList (the adaptive launch tested once per call) */
              PT_MODE_ADAPTIVE };    /* one pixel per lane over the packed live pixels (the host has run pt_launch_live_list on the same stream) */

/* the shape of a launch: what the launcher reads off its arguments */
struct PtShape {
    int mode;
    bool groups;       /* TbDeviceTargets::samples: frame groups */
    bool list;         /* TbDeviceTargets::liveList (PT_MODE_ADAPTIVE: and liveCount) */
    bool counting;     /* ray counters */
    bool sceneLds, twoLevel, layoutC;
    bool split, overflowFits; /* split stack (TbDeviceScene::stackOverflow); its columns cover the largest resident grid: 2 x 8 workgroups per CU */
    bool hits, first;  /* TbDeviceTargets::primaryHits: the pre-pass's hit records; ::firstBounce: first-bounce records in their place */
    bool shrinking;    /* TbDeviceTargets::fgGuided: the host asks for groups that shrink over the end of the launch */
};

enum PtPre { PT_PRE_NONE = 0, PT_PRE_PRIMARY /* pt_primary<F, hybrid, nodeC> */, PT_PRE_FIRST /* pt_first<F, hybrid> */ };
/* a kernel by its template arguments: pt_stream<F, sceneLds, count> where `stream`, else pt_persistent<F, sceneLds, count, groups, hybrid, nodeC,
 * twoLevel, primary, first, guided, adaptive>; `pre` runs first on the same stream */
struct PtForm {
    bool stream, sceneLds, count, groups, hybrid, nodeC, twoLevel, primary, first, guided, adaptive; int pre;
    constexpr uint32_t code() const { return (uint32_t)stream | sceneLds << 1 | count << 2 | groups << 3 | hybrid << 4 | nodeC << 5 | twoLevel << 6 | primary << 7 |
        first << 8 | guided << 9 | adaptive << 10 | (uint32_t)pre << 11; }
};
constexpr PtForm pt_form_of(uint32_t c) { return PtForm{(c & 1) != 0, (c & 2) != 0, (c & 4) != 0, (c & 8) != 0, (c & 16) != 0, (c & 32) != 0, (c & 64) != 0,
    (c & 128) != 0, (c & 256) != 0, (c & 512) != 0, (c & 1024) != 0, (int)(c >> 11)}; }
constexpr uint32_t PT_FORM_CODES = 3u << 11;

struct PtPick { bool ok; PtForm form; }; /* !ok: the launcher answers hipErrorInvalidValue */

/* groups that shrink over the end of the launch are compiled into the frame-group kernels of scenes in LDS only (a copy of its own, pt_persistent.inc
 * GUIDED); every other launch has equal groups whatever the host asked for -- the host asks for it there only */
constexpr bool pt_shrinking_groups(const PtShape& s) { return s.groups && s.shrinking && s.sceneLds && !s.split && !s.twoLevel && !s.layoutC && !s.hits; }

/* Which kernel of copy `c` runs a launch of shape `s`, or none. */
constexpr PtPick pt_pick_form(const PtCopy& c, const PtShape& s, bool profileGroups = PT_PROFILE_GROUPS)
{
    const PtPick refuse{false, PtForm{}};
    const bool base = c.role == PT_ROLE_BASE, occupancy = c.role == PT_ROLE_OCCUPANCY;
    PtForm f{}; f.sceneLds = s.sceneLds;
    if (s.mode == PT_MODE_ADAPTIVE) { /* the base copy's one-pixel-per-lane form over the live pixels; whole stack in LDS, layout B */
        if (!base || !s.list || s.groups || s.hits || s.counting || s.split || s.layoutC || (s.twoLevel && !c.ext())) return refuse;
        f.adaptive = true; return PtPick{true, f};
    }
    if (s.mode == PT_MODE_LIVE_GROUPS) { /* no counters, no hit records, layout B, equal groups */
        if (!s.groups || !s.list || s.counting || s.hits || s.layoutC || s.shrinking) return refuse;
        if (occupancy ? (s.split && !s.overflowFits) || (s.twoLevel && s.sceneLds) : s.split || (s.twoLevel && !c.ext())) return refuse;
        if (c.role == PT_ROLE_LDS_GROUPS && !s.sceneLds) return refuse;
        f.groups = f.adaptive = true; f.hybrid = s.split; f.twoLevel = occupancy && s.twoLevel;
        return PtPick{true, f};
    }
    const bool stream = s.mode == PT_MODE_STREAM;
    if (s.groups && (s.counting || stream)) return refuse; /* frame groups: pt_persistent without counters only */
    const bool guided = pt_shrinking_groups(s);
    if (c.role == PT_ROLE_LDS_GROUPS) {
        if (!s.groups || !s.sceneLds || s.twoLevel || s.hits || s.layoutC || s.split) return refuse;
        f.groups = true; f.guided = guided; return PtPick{true, f};
    }
    if (stream && !c.streaming) return refuse;
    if (s.counting) { if (!c.counting) return refuse; f.stream = stream; f.count = true; return PtPick{true, f}; }
    if (s.twoLevel && occupancy) { /* the tuned two-level walk lives in the frame-group kernels of this copy */
        if (!s.groups || s.sceneLds || s.layoutC || (s.split && !s.overflowFits)) return refuse;
        f.groups = f.twoLevel = true; f.hybrid = s.split; return PtPick{true, f};
    }
    if (s.twoLevel && !c.ext()) return refuse; /* of the base copies only the full feature set walks two levels */
    if (s.hits) { /* frame-group kernels, scenes fetched from memory, one level; the pre-pass has the stack layout of the kernel it feeds */
        if (!c.prepass() || !s.groups || s.sceneLds || s.twoLevel || (s.split && !s.overflowFits)) return refuse;
        if (base && (s.split || s.layoutC)) return refuse; /* a base copy: whole stack in LDS, layout B */
        if (s.first && s.layoutC) return refuse;           /* first-bounce records: layout B only */
        f.groups = f.primary = true; f.hybrid = s.split; f.first = s.first; f.nodeC = s.layoutC; f.pre = s.first ? PT_PRE_FIRST : PT_PRE_PRIMARY;
        return PtPick{true, f};
    }
    if (s.layoutC) { /* compiled into the frame-group kernels of the occupancy copies, scenes fetched from memory */
        if (!occupancy || !s.groups || s.sceneLds || (s.split && !s.overflowFits)) return refuse;
        f.groups = f.nodeC = true; f.hybrid = s.split; return PtPick{true, f};
    }
    if (s.split) { /* the tree is deeper than this copy's share of LDS; the host sized the overflow for a resident grid */
        if (!occupancy || !s.groups || !s.overflowFits) return refuse;
        f.groups = f.hybrid = true; return PtPick{true, f};
    }
    if (s.groups) { f.groups = true; if (profileGroups) f.count = true; else if (guided) f.guided = true; return PtPick{true, f}; }
    f.stream = stream; return PtPick{true, f};
}

constexpr PtShape pt_shape_of(uint32_t i) /* the i-th of PT_SHAPES shapes: every combination of the fields */
{
    return PtShape{(int)(i & 3u), (i & 4u) != 0, (i & 8u) != 0, (i & 16u) != 0, (i & 32u) != 0, (i & 64u) != 0, (i & 128u) != 0, (i & 256u) != 0,
        (i & 512u) != 0, (i & 1024u) != 0, (i & 2048u) != 0, (i & 4096u) != 0};
}
constexpr uint32_t PT_SHAPES = 8192u;

/* the kernels a copy can launch at all: what its unit instantiates, no more */
struct PtFormSet { uint32_t code[64]; int n; };
constexpr PtFormSet pt_forms_of(const PtCopy& c, bool profileGroups = PT_PROFILE_GROUPS)
{
    PtFormSet set{}; bool seen[PT_FORM_CODES] = {};
    for (uint32_t i = 0; i < PT_SHAPES; i++) {
        const PtPick p = pt_pick_form(c, pt_shape_of(i), profileGroups);
        if (p.ok && !seen[p.form.code()]) { seen[p.form.code()] = true; set.code[set.n++] = p.form.code(); }
    }
    return set;
}
