// csrc/ctx_state.hpp and csrc/handles.hpp on their own (no HIP): the raw device memory is malloc / free with a
// count of live bytes and blocks, so a leak, a double free or a lost buffer shows in the counters (and in the
// sanitized build); pinned memory and events likewise.  Checks DevBuf's alloc / reset / move / assign, arrays of
// handles, PinBuf and Event (create over a live event, moves, reset, a growing vector), and that assigning a
// default MeshState / PartitionState to a filled one frees everything and restores the values the mesh
// teardown used to write field by field.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <utility>
#include <vector>

#include "ctx_state.hpp"

using namespace cdfem;

static std::map<void *, size_t> live;  // block -> bytes
static size_t live_bytes = 0;
static int fails = 0;

void *cdfem::raw_device_alloc(size_t bytes)
{
    void *p = std::malloc(bytes);
    if (!p) throw std::bad_alloc();
    live[p] = bytes;
    live_bytes += bytes;
    return p;
}
void cdfem::raw_device_free(void *p) noexcept
{
    auto it = live.find(p);
    if (it == live.end()) {
        std::printf("FAIL: free of a block that is not live\n");
        ++fails;
        return;
    }
    live_bytes -= it->second;
    live.erase(it);
    std::free(p);
}

// pinned memory and events: the same counting, kept apart so that a handle released through the wrong function
// shows; an event is a one-byte block
static std::map<void *, size_t> live_pinned;
static int live_events = 0;
void *cdfem::raw_pinned_alloc(size_t bytes)
{
    void *p = std::malloc(bytes);
    if (!p) throw std::bad_alloc();
    live_pinned[p] = bytes;
    return p;
}
void cdfem::raw_pinned_free(void *p) noexcept
{
    if (live_pinned.erase(p) != 1) {
        std::printf("FAIL: pinned free of a block that is not live\n");
        ++fails;
        return;
    }
    std::free(p);
}
static bool last_event_timing = false;
ihipEvent_t *cdfem::raw_event_create(bool timing)
{
    void *p = std::malloc(1);
    if (!p) throw std::bad_alloc();
    ++live_events;
    last_event_timing = timing;
    return static_cast<ihipEvent_t *>(p);
}
void cdfem::raw_event_destroy(ihipEvent_t *e) noexcept
{
    --live_events;
    std::free(e);
}

#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);      \
            ++fails;                                                 \
        }                                                            \
    } while (0)

static const auto host_copy = [](void *dst, const void *src, size_t bytes) { std::memcpy(dst, src, bytes); };

static void check_devbuf()
{
    {
        DevBuf<double> a;
        CHECK(!a && a.get() == nullptr && a.size() == 0 && a == nullptr);
        a.alloc(10);
        CHECK(a && a.size() == 10 && live_bytes == 80 && live.size() == 1);
        double *first = a;
        a.alloc(3);  // over a live buffer: the old block is freed
        CHECK(a.size() == 3 && live_bytes == 24 && live.size() == 1 && live.count(first) == 0);
        a.alloc(0);  // one element, as a zero-size device allocation does
        CHECK(a != nullptr && a.size() == 0 && live_bytes == 8);
        a.reset();
        CHECK(!a && a.size() == 0 && live_bytes == 0);
        a.reset();  // twice is harmless
        CHECK(live_bytes == 0);

        a.alloc(4);
        const double *raw = a;
        DevBuf<double> b(std::move(a));  // move construction
        CHECK(!a && a.size() == 0 && b.get() == raw && b.size() == 4 && live_bytes == 32);
        DevBuf<double> c;
        c.alloc(7);
        c = std::move(b);  // move assignment over a live buffer
        CHECK(!b && c.get() == raw && c.size() == 4 && live_bytes == 32 && live.size() == 1);
        DevBuf<double> &self = c;
        c = std::move(self);  // self-move keeps the buffer
        CHECK(c.get() == raw && c.size() == 4 && live_bytes == 32);
        c[1] = 2.5;  // pointer idioms through the implicit conversion
        const double *off = c + 1;
        CHECK(*off == 2.5 && off - 1 == raw);

        const std::vector<int> v{3, 1, 4, 1, 5};
        DevBuf<int> d;
        d.alloc(100);
        d.assign(v, host_copy);
        CHECK(d.size() == 5 && live_bytes == 32 + 20 && std::memcmp(d, v.data(), 20) == 0);
        d.assign(std::vector<int>{}, host_copy);  // empty: allocated, nothing copied
        CHECK(d != nullptr && d.size() == 0 && live_bytes == 32 + 4);
        d.assign(v.data() + 1, 2, host_copy);
        CHECK(d.size() == 2 && d[0] == 1 && d[1] == 4);
    }  // c and d go out of scope
    CHECK(live_bytes == 0 && live.empty());

    {
        DevBuf<double> w[8];  // arrays of handles
        for (auto &b : w) b.alloc(5);
        CHECK(live_bytes == 8 * 40 && live.size() == 8);
        w[3].reset();
        CHECK(live_bytes == 7 * 40);
        struct Holder {
            DevBuf<double> w[8];
            int n = 1;
        } h, fresh;
        for (auto &b : h.w) b.alloc(2);
        h.n = 9;
        h = Holder{};
        CHECK(live_bytes == 7 * 40 && h.n == 1 && !h.w[0] && !h.w[7]);
        (void)fresh;
    }
    CHECK(live_bytes == 0 && live.empty());
}

static void check_pinned_and_events()
{
    {
        struct Slot {
            int done;
            int its;
        };
        PinBuf<Slot> a, b;  // a poll slot array, read through operator->
        a.alloc(3);
        CHECK(a && a.size() == 3 && live_pinned.size() == 1 && live_pinned.begin()->second == 24 && live.empty());
        a[0] = Slot{1, 7};
        CHECK(a->done == 1 && a->its == 7);
        b = std::move(a);
        CHECK(!a && b.size() == 3 && live_pinned.size() == 1);
        b.alloc(5);
        CHECK(live_pinned.size() == 1 && live_pinned.begin()->second == 40);
    }
    CHECK(live_pinned.empty());
    {
        Event e;
        CHECK(!e && e.get() == nullptr && live_events == 0);
        e.create(false);
        CHECK(e && live_events == 1 && !last_event_timing);
        ihipEvent_t *raw = e;
        e.create(true);  // over a live event: the old one is destroyed
        CHECK(e && live_events == 1 && last_event_timing);
        raw = e;
        Event f(std::move(e));  // move construction
        CHECK(!e && f.get() == raw && live_events == 1);
        Event g;
        g.create(false);
        g = std::move(f);  // move assignment over a live event
        CHECK(!f && g.get() == raw && live_events == 1);
        Event &self = g;
        g = std::move(self);
        CHECK(g.get() == raw && live_events == 1);
        g.reset();
        g.reset();
        CHECK(!g && live_events == 0);
        std::vector<Event> v;  // the profiling slots: a vector that grows moves its events
        for (int i = 0; i < 9; ++i) v.emplace_back().create(true);
        Event pair[2];
        for (auto &p : pair) p.create(false);
        CHECK(live_events == 11);
    }
    CHECK(live_events == 0);
}

static void fill(FaDeviceState &f)
{
    f.nnz = 11;
    f.nslices = 12;
    f.nstored = 13;
    f.sell_nnz_wide = 14;
    f.lds_rows = 15;
    f.lds_max = 16;
    f.sell_lpr = 4;
    f.sell_windowed = true;
    for (DevBuf<int32_t> *b : {&f.d_rowptr, &f.d_cols, &f.d_diagpos, &f.d_coff, &f.d_cpos, &f.d_sptr, &f.d_srows,
                               &f.d_scols, &f.d_smap, &f.d_hptr, &f.d_hidx, &f.d_rperm})
        b->alloc(6);
    for (DevBuf<double> *b : {&f.d_vals, &f.d_vals_c, &f.d_Ee, &f.d_svals, &f.d_svals_c, &f.d_pv[0], &f.d_pv[1]})
        b->alloc(6);
    f.d_sdel.alloc(6);
    f.d_swide.alloc(6);
    f.d_sloc.alloc(6);
}

static void check_fa_default(const FaDeviceState &f)
{
    CHECK(f.nnz == 0 && f.nslices == 0 && f.nstored == 0 && f.sell_nnz_wide == 0 && f.lds_rows == 0 && f.lds_max == 0);
    CHECK(f.sell_lpr == 1 && !f.sell_windowed);
    CHECK(!f.d_rowptr && !f.d_cols && !f.d_diagpos && !f.d_coff && !f.d_cpos && !f.d_vals && !f.d_vals_c && !f.d_Ee);
    CHECK(!f.d_sptr && !f.d_srows && !f.d_scols && !f.d_smap && !f.d_sdel && !f.d_swide && !f.d_hptr && !f.d_hidx);
    CHECK(!f.d_sloc && !f.d_rperm && !f.d_pv[0] && !f.d_pv[1] && !f.d_svals && !f.d_svals_c);
}

static void check_mesh_state()
{
    MeshState m;
    fill(m);
    m.mesh_ready = m.structured = m.epencil = m.fa_ready = m.pa_ready = m.dinv_ready = true;
    m.hb_nblk = 21;
    m.den_grp = 8;
    m.slab_nl_max = 22;
    m.slab_nb_max = 23;
    m.zlo_shared = m.zhi_shared = 1;
    m.geom = 1;
    m.ktab_key = 196;
    m.h_verts.assign(9, 1.0);
    m.h_sxi_d.assign(3, 1.0);
    m.h_sxi_cm.assign(3, 1.0);
    m.h_sxi_lf.assign(3, 1.0);
    for (DevBuf<double> *b :
         {&m.d_verts, &m.d_hbpart, &m.d_gsum, &m.d_uelem, &m.d_udiag, &m.d_hoelem, &m.d_face, &m.d_ones, &m.d_dalt,
          &m.d_stab, &m.d_stab_lf, &m.d_tpart, &m.d_ktab, &m.d_bsum, &m.d_small, &m.d_dinv_p, &m.d_qd, &m.d_qaff,
          &m.d_geom, &m.d_hgeom, &m.d_Ye, &m.d_dinv, &m.d_part, &m.d_gm, &m.d_gm_part, &m.d_lfq, &m.d_bcgs,
          &m.d_bcgs_part})
        b->alloc(5);
    for (auto &b : m.d_w) b.alloc(5);
    for (auto &b : m.d_if) b.alloc(5);
    for (DevBuf<int32_t> *b : {&m.d_map, &m.d_e2l_off, &m.d_e2l_pos, &m.d_ess_list, &m.d_perm}) b->alloc(5);
    m.d_ess.alloc(5);
    m.d_bess.alloc(5);
    m.d_gcnt.alloc(5);
    CHECK(live.size() == 22 + 28 + 8 + 4 + 5 + 3);

    // a pattern built aside and moved in whole (cdfem_fa_setup) replaces the one held
    FaDeviceState f;
    fill(f);
    f.nnz = 99;
    static_cast<FaDeviceState &>(m) = std::move(f);
    CHECK(m.nnz == 99 && m.d_rowptr && !f.d_rowptr && live.size() == 22 + 28 + 8 + 4 + 5 + 3);

    m = MeshState{};  // what the mesh teardown does
    CHECK(live_bytes == 0 && live.empty());
    check_fa_default(m);
    CHECK(!m.mesh_ready && !m.structured && !m.epencil && !m.fa_ready && !m.pa_ready && !m.dinv_ready);
    CHECK(m.hb_nblk == 0 && m.den_grp == 1 && m.slab_nl_max == 0 && m.slab_nb_max == 0);
    CHECK(m.zlo_shared == 0 && m.zhi_shared == 0 && m.geom == 0 && m.ktab_key == -1);
    CHECK(m.h_verts.empty() && m.h_sxi_d.empty() && m.h_sxi_cm.empty() && m.h_sxi_lf.empty());
    CHECK(!m.d_verts && !m.d_map && !m.d_w[0] && !m.d_w[7] && !m.d_if[3] && !m.d_bcgs && !m.d_gcnt && !m.d_bess);
}

static void check_partition_state()
{
    PartitionState p;
    p.part_mode = 2;
    p.skip_lo = 17;
    p.n_shd = 5;
    p.nbr_rank = {1, 3};
    p.nbr_off = {0, 2, 5};
    p.h_sh_idx = {0, 1, 2, 3, 4};
    for (DevBuf<int32_t> *b : {&p.d_sh_idx, &p.d_shd, &p.d_shd_off, &p.d_shd_src, &p.d_shd_owner}) b->alloc(5);
    p.d_sh_send.alloc(5);
    p.d_sh_recv.alloc(5);
    CHECK(live.size() == 7);
    p = PartitionState{};  // partition_free
    CHECK(live_bytes == 0 && live.empty());
    CHECK(p.part_mode == 0 && p.skip_lo == 0 && p.n_shd == 0);
    CHECK(p.nbr_rank.empty() && p.nbr_off.empty() && p.h_sh_idx.empty());
    CHECK(!p.d_sh_idx && !p.d_shd && !p.d_shd_off && !p.d_shd_src && !p.d_shd_owner && !p.d_sh_send && !p.d_sh_recv);
}

int main()
{
    check_devbuf();
    check_pinned_and_events();
    check_mesh_state();
    check_partition_state();
    if (fails) {
        std::printf("ctx state FAILED: %d checks\n", fails);
        return 1;
    }
    std::printf("ctx state ok\n");
    return 0;
}
