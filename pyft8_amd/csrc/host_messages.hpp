// host_messages.hpp -- native host message layer: 77-bit words -> strings, call hashes, duplicate filter (decoders.py:16-115, databases.py:10-26, receiver.py:51-66)
// Part of libft8rx.so; included by ft8rx.hip.  Pure host C++ (needs only include/ft8rx.h and ft8_tables.h): it is also compiled on
// its own by g++ -fsanitize=address,undefined for the host sanitizer target (oracle/Makefile `asan`, tests/host_asan_driver.cpp).
#ifndef FT8RX_HOST_MESSAGES_HPP
#define FT8RX_HOST_MESSAGES_HPP

// ====================================================================================== host message layer (native)
// C++ twin of pyft8_amd/messages.py: 77-bit payload -> text (reference decoders.py:16-115), call-hash table
// (databases.py:8-26) and the per-frame replay of records/events in the reference's emit order with its duplicate
// filter (receiver.py:51-66, 389-398).  Pure host code, no HIP: frames are independent and are packaged by a pool
// of threads so that the Python surface is not the bottleneck behind ~26 k decoded frames/s.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>
#include <thread>
#include <unordered_map>
#include <condition_variable>
#include <functional>
#include <unistd.h>
#include "ft8_msg_tables.h"
namespace hostmsg {
// Persistent worker threads of the packaging entry points.  Creating and joining n std::threads per call was ~1 ms of the 1.2 ms a
// 256-frame batch took at 32 threads (and, with one process per GPU, tens of thousands of thread creations per second on the host).
// run(n, fn) executes fn on up to n threads -- the caller and pool threads 1 .. n - 1 (created on first need, detached, parked on a
// condition variable between calls); fn must hand out its own work (an atomic counter) and return when none is left.  The caller
// returns when its own fn has returned and every pool thread that ENTERED fn has left it: a pool thread that wakes up late (a loaded
// host) finds the run closed and is not waited for.  One run at a time per process; the state is never freed (threads may still be
// parked on it at exit) and is rebuilt in a forked child, whose copy of it has no threads behind it.
class HostPool {
    struct State {
        std::mutex run_m, m;
        std::condition_variable cv_go, cv_done;
        const std::function<void(int)>* job = nullptr;
        int n_threads = 0, job_n = 0, entered = 0, exited = 0;
        bool open = false;
        uint64_t gen = 0;
        pid_t pid = 0;
    };
    static State*& state() { static State* st = nullptr; return st; }
    static void worker(State* st, int idx) {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(st->m);
        for (;;) {
            st->cv_go.wait(lk, [&] { return st->gen != seen; });
            seen = st->gen;
            if (st->open && idx < st->job_n) {
                const std::function<void(int)>* j = st->job;
                st->entered++;
                lk.unlock();
                (*j)(idx);
                lk.lock();
                if (++st->exited == st->entered) st->cv_done.notify_one();
            }
        }
    }
public:
    static void run(int n, const std::function<void(int)>& fn) {
        if (n <= 1) { fn(0); return; }
        static std::mutex create_m;
        State* st;
        {
            std::lock_guard<std::mutex> g(create_m);
            if (!state() || state()->pid != getpid()) { state() = new State; state()->pid = getpid(); }
            st = state();
        }
        std::lock_guard<std::mutex> g(st->run_m);
        {
            std::unique_lock<std::mutex> lk(st->m);
            while (st->n_threads < n - 1) { const int idx = ++st->n_threads; std::thread(worker, st, idx).detach(); }
            st->job = &fn; st->job_n = n; st->entered = st->exited = 0; st->open = true; st->gen++;
        }
        st->cv_go.notify_all();
        fn(0);
        std::unique_lock<std::mutex> lk(st->m);
        st->open = false;                                           // nobody enters from here on
        st->cv_done.wait(lk, [&] { return st->exited == st->entered; });
        st->job = nullptr; st->job_n = 0;
    }
};
// optional reject log: the reference appends every call that fails simple_validate_call to 'rejected_callsigns.txt' in the
// working directory (decoders.py:114-115).  Off by default; ft8rx_set_reject_log(path) turns it on for the process.
static std::string g_reject_log;
static std::mutex g_reject_mu;
static std::atomic<bool> g_reject_on{false};      // the packaging threads' fast path; the path string itself is only read under the mutex
static void set_reject_log(const char* path) {
    std::lock_guard<std::mutex> lk(g_reject_mu);
    g_reject_log = path ? path : "";
    g_reject_on.store(!g_reject_log.empty(), std::memory_order_release);
}
static void log_reject(const std::string& call) {
    if (!g_reject_on.load(std::memory_order_acquire)) return;
    std::lock_guard<std::mutex> lk(g_reject_mu);
    if (g_reject_log.empty()) return;
    if (FILE* f = fopen(g_reject_log.c_str(), "a")) { fprintf(f, "%s\n", call.c_str()); fclose(f); }
}
static const char A37[] = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ";
static const char A38[] = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ/";
static const char A27[] = " ABCDEFGHIJKLMNOPQRSTUVWXYZ";
// The call-hash table (databases.py:8-26): key = (number of hash bits, hash) -> callsign, last writer wins.  An open-addressing
// table of fixed 24-byte entries: every valid callsign of every replayed unpack() call is entered under three keys, so a node-based
// map spent most of the message layer's time in its allocator.
struct Hashes {
    struct Entry { uint64_t key; char call[15]; uint8_t len; };   // len = 0xFF: empty slot (keys themselves may be any value)
    std::vector<Entry> tab;
    size_t used = 0;
    Hashes() { tab.resize(1024); clear(); }
    void clear() { for (auto& e : tab) e.len = 0xFF; used = 0; }
    size_t size() const { return used; }
    static size_t slot_of(uint64_t key, size_t cap) { return (size_t)((key * 0x9E3779B97F4A7C15ULL) >> 32) & (cap - 1); }
    void put(uint64_t key, const std::string& call) {
        if (2 * (used + 1) > tab.size()) {                        // keep the load factor <= 1/2
            std::vector<Entry> old; old.swap(tab);
            tab.resize(old.size() * 2); clear();
            for (const auto& e : old) if (e.len != 0xFF) put(e.key, std::string(e.call, e.len));
        }
        size_t i = slot_of(key, tab.size());
        while (tab[i].len != 0xFF && tab[i].key != key) i = (i + 1) & (tab.size() - 1);
        if (tab[i].len == 0xFF) used++;
        tab[i].key = key;
        tab[i].len = (uint8_t)(call.size() < sizeof(tab[i].call) ? call.size() : sizeof(tab[i].call));
        memcpy(tab[i].call, call.data(), tab[i].len);
    }
    void add(const std::string& call) {
        uint64_t acc = 0;
        for (int i = 0; i < 11; i++) {
            char ch = i < (int)call.size() ? call[i] : ' ';
            const char* q = strchr(A38, ch);
            int64_t idx = (q && ch) ? (int64_t)(q - A38) : -1;
            acc = acc * 38 + (uint64_t)idx;
        }
        acc *= 47055833459ULL;
        const int nb[3] = {10, 12, 22};
        for (int k = 0; k < 3; k++) put(((uint64_t)nb[k] << 32) | (acc >> (64 - nb[k])), call);
    }
    std::string get(uint32_t h, int nb) const {
        const uint64_t key = ((uint64_t)nb << 32) | h;
        size_t i = slot_of(key, tab.size());
        while (tab[i].len != 0xFF) { if (tab[i].key == key) return std::string(tab[i].call, tab[i].len); i = (i + 1) & (tab.size() - 1); }
        return std::string("...");
    }
};
static std::string strip(const std::string& t) {
    size_t a = 0, b = t.size();
    while (a < b && t[a] == ' ') a++;
    while (b > a && t[b - 1] == ' ') b--;
    return t.substr(a, b - a);
}
static bool plausible(const std::string& c) {
    if (c.size() < 3 || c.find(' ') != std::string::npos) return false;
    auto dig = [](char x) { return x >= '0' && x <= '9'; };
    auto a36 = [](char x) { return (x >= '0' && x <= '9') ? x - '0' : (x >= 'A' && x <= 'Z') ? x - 'A' + 10 : -1; };
    if (c[0] >= 'A' && c[0] <= 'Z' && ((FT8_PFX1_MASK >> (c[0] - 'A')) & 1u) && dig(c[1]))
        if (!(((FT8_PFX1_TRAP >> (c[0] - 'A')) & 1u) && dig(c[2]))) return true;
    int x0 = a36(c[0]), x1 = a36(c[1]);
    return x0 >= 0 && x1 >= 0 && ((FT8_PFX2[x0] >> x1) & 1ULL) && dig(c[2]);
}
static bool validate(const std::string& c) { const bool ok = plausible(c); if (!ok) log_reject(c); return ok; }
static bool field29(uint32_t v29, int i3, Hashes& H, std::string& out) {
    const uint32_t flag = v29 & 1u, n28 = v29 >> 1;
    char buf[24];
    if (n28 < 3) { out = n28 == 0 ? "DE" : n28 == 1 ? "QRZ" : "CQ"; return true; }
    if (n28 < 1004) { snprintf(buf, sizeof buf, "CQ %03u", n28 - 3); out = buf; return true; }
    if (n28 < 21443) {
        uint32_t v = n28 - 1003; std::string t(4, ' ');
        for (int i = 3; i >= 0; i--) { t[i] = A27[v % 27]; v /= 27; }
        out = "CQ " + strip(t); return true;
    }
    if (n28 < 2063592u + 4194303u) { out = "<" + H.get(n28 - 2063592u, 22) + ">"; return true; }
    std::string call;
    int64_t v = (int64_t)n28 - (2063592 + 4194304);
    if (v < 0) call = "ZZ9ZZZ";                                   // negative-index artefact of the reference at n28 = 6257895
    else {
        char ch[7]; ch[6] = 0;
        ch[5] = A27[v % 27]; v /= 27; ch[4] = A27[v % 27]; v /= 27; ch[3] = A27[v % 27]; v /= 27;
        ch[2] = (char)('0' + v % 10); v /= 10; ch[1] = A37[1 + v % 36]; v /= 36; ch[0] = A37[v % 37];
        call = strip(ch);
    }
    if (!validate(call)) return false;
    if (flag) {
        call += (i3 == 2) ? "/P" : "/R";
        if (i3 != 2 && !(call[0] == 'A' || call[0] == 'K' || call[0] == 'N' || call[0] == 'W')) return false;
    }
    H.add(call);
    out = call;
    return true;
}
// unpack(): true + 3 fields when the reference returns a tuple; mutates H exactly like the reference
static bool unpack(uint64_t lo, uint64_t hi, Hashes& H, std::string f[3]) {
    if (!lo && !hi) return false;
    const unsigned i3 = (unsigned)(lo & 7u);
    if (i3 == 1 || i3 == 2) {
        const uint32_t g16 = (uint32_t)((lo >> 3) & 0xFFFFu), cb = (uint32_t)((lo >> 19) & 0x1FFFFFFFu);
        const uint32_t ca = (uint32_t)(((lo >> 48) | (hi << 16)) & 0x1FFFFFFFu), g15 = g16 & 0x7FFFu;
        if (g15 == 0) return false;
        char g[16];
        if (g15 < 32400) { unsigned q = g15 / 1800, r = g15 % 1800; g[0] = (char)('A' + q); g[1] = (char)('A' + r / 100); g[2] = (char)('0' + (r % 100) / 10); g[3] = (char)('0' + r % 10); g[4] = 0; }
        else if (g15 <= 32404) { static const char* T5[5] = {"", "", "RRR", "RR73", "73"}; snprintf(g, sizeof g, "%s", T5[g15 - 32400]); }
        else snprintf(g, sizeof g, "%s%+03d", (g16 >> 15) ? "R" : "", (int)g15 - 32435);
        const bool oka = field29(ca, (int)i3, H, f[0]);
        const bool okb = field29(cb, (int)i3, H, f[1]);
        f[2] = g;
        return oka && okb && g[0] != 0;
    }
    if (i3 == 4) {
        const unsigned cq = (unsigned)((lo >> 3) & 1u), rrr = (unsigned)((lo >> 4) & 3u), swp = (unsigned)((lo >> 6) & 1u);
        uint64_t n58 = ((lo >> 7) | (hi << 57)) & ((1ULL << 58) - 1);
        const uint32_t h12 = (uint32_t)((hi >> 1) & 0xFFFu);
        if ((cq != 0) == (rrr != 0)) return false;
        std::string first = cq ? std::string("CQ") : "<" + H.get(h12, 12) + ">";
        std::string t(12, ' ');
        for (int i = 11; i >= 0; i--) { t[i] = A38[n58 % 38]; n58 /= 38; }
        t = strip(t);
        H.add(t);
        static const char* R4[4] = {"", "RRR", "RR73", "73"};
        f[0] = swp ? t : first; f[1] = swp ? first : t; f[2] = R4[rrr];
        return true;
    }
    return false;
}
// unpack() with the opt-in message types of `mask` (FT8RX_MT_* bits, include/ft8rx.h): the C++ twin of messages.unpack_ext.  mask = 0
// and i3 = 1, 2, 4 are unpack() itself.  true iff the device gate ft8_valid77_ext (csrc/ft8_dev.h) accepts the word outside OSD; the
// c28 fields go through field29 (a standard call enters H, as the reference's call_29 does for i3 = 1 / 2), both before any range check,
// so H evolves the same way whatever the outcome; hash fields are looked up in H ("<...>" on a miss).
static bool unpack_ext(uint64_t lo, uint64_t hi, unsigned mask, Hashes& H, std::string f[3]) {
    const unsigned i3 = (unsigned)(lo & 7u), n3 = (unsigned)((lo >> 3) & 7u);
    if (mask == 0 || (!lo && !hi) || i3 == 1 || i3 == 2 || i3 == 4) return unpack(lo, hi, H, f);
    typedef unsigned __int128 u128;
    const u128 w = ((u128)(hi & 0x1FFFull) << 64) | lo;
    auto bits = [&](int pos, int n) { return (uint64_t)((w >> pos) & (((u128)1 << n) - 1)); };
    char buf[48];
    auto hashed = [&](uint32_t h, int nb) { return "<" + H.get(h, nb) + ">"; };
    if (i3 == 0) {
        const u128 v71 = w >> 6;
        if (n3 == 0) {                                                  // free text: 13 characters, base 42, first character most significant
            static const char A42[] = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ+-./?";
            if (!(mask & FT8RX_MT_FREE_TEXT)) return false;
            u128 v = v71;
            const u128 lim = ((u128)0x44 << 64) | 0x9979e458016ca000ull;  // 42^13
            if (v >= lim) return false;
            std::string t(13, ' ');
            for (int i = 12; i >= 0; i--) { t[i] = A42[(int)(v % 42)]; v /= 42; }
            f[0] = strip(t); f[1] = ""; f[2] = "";
            return true;
        }
        if (n3 == 5) {                                                  // telemetry: 18 hex digits, leading zeros dropped
            if (!(mask & FT8RX_MT_TELEMETRY) || v71 == 0) return false;
            snprintf(buf, sizeof buf, "%X%016llX", (unsigned)(uint64_t)(v71 >> 64), (unsigned long long)(uint64_t)v71);
            const char* q = buf; while (*q == '0') q++;
            f[0] = q; f[1] = ""; f[2] = "";
            return true;
        }
        if (n3 == 1) {                                                  // DXpedition: c28 c28 h10 r5
            if (!(mask & FT8RX_MT_DXPEDITION)) return false;
            std::string a, b;
            const bool oka = field29((uint32_t)bits(49, 28) << 1, 1, H, a), okb = field29((uint32_t)bits(21, 28) << 1, 1, H, b);
            snprintf(buf, sizeof buf, " %+03d", 2 * (int)bits(6, 5) - 30);
            f[0] = a + " RR73;"; f[1] = b; f[2] = hashed((uint32_t)bits(11, 10), 10) + buf;
            return oka && okb;
        }
        if (n3 == 3 || n3 == 4) {                                       // ARRL Field Day: c28 c28 R1 n4 k3 s7
            if (!(mask & FT8RX_MT_FIELD_DAY)) return false;
            std::string a, b;
            const bool oka = field29((uint32_t)bits(49, 28) << 1, 1, H, a), okb = field29((uint32_t)bits(21, 28) << 1, 1, H, b);
            const unsigned s7 = (unsigned)bits(6, 7);
            if (!oka || !okb || s7 < 1 || s7 > FT8_N_SECTIONS) return false;
            snprintf(buf, sizeof buf, "%s%d%c %s", bits(20, 1) ? "R " : "", (int)bits(16, 4) + 1 + (n3 == 4 ? 16 : 0), (char)('A' + bits(13, 3)),
                     FT8_SECTIONS[s7 - 1]);
            f[0] = a; f[1] = b; f[2] = buf;
            return true;
        }
        return false;
    }
    if (i3 == 3) {                                                      // ARRL RTTY Roundup: t1 c28 c28 R1 r3 s13
        if (!(mask & FT8RX_MT_RTTY_RU)) return false;
        std::string a, b;
        const bool oka = field29((uint32_t)bits(48, 28) << 1, 1, H, a), okb = field29((uint32_t)bits(20, 28) << 1, 1, H, b);
        const unsigned s13 = (unsigned)bits(3, 13);
        const bool serial = s13 >= 1 && s13 <= 7999, mult = s13 >= 8001 && s13 <= 8000 + FT8_N_MULT;
        if (!oka || !okb || !(serial || mult)) return false;
        char ex[8];
        if (serial) snprintf(ex, sizeof ex, "%04u", s13); else snprintf(ex, sizeof ex, "%s", FT8_MULT[s13 - 8001]);
        snprintf(buf, sizeof buf, "%s5%d9 %s", bits(19, 1) ? "R " : "", (int)bits(16, 3) + 2, ex);
        f[0] = (bits(76, 1) ? "TU; " : "") + a; f[1] = b; f[2] = buf;
        return true;
    }
    if (i3 == 5) {                                                      // EU VHF contest: h12 h22 R1 r3 s11 g25
        if (!(mask & FT8RX_MT_EU_VHF)) return false;
        uint32_t g = (uint32_t)bits(3, 25);
        if (g >= 18662400u) return false;
        char loc[7]; loc[6] = 0;
        loc[5] = (char)('A' + g % 24); g /= 24; loc[4] = (char)('A' + g % 24); g /= 24; loc[3] = (char)('0' + g % 10); g /= 10;
        loc[2] = (char)('0' + g % 10); g /= 10; loc[1] = (char)('A' + g % 18); g /= 18; loc[0] = (char)('A' + g);
        snprintf(buf, sizeof buf, "%s%02d%04u %s", bits(42, 1) ? "R " : "", 52 + (int)bits(39, 3), (unsigned)bits(28, 11), loc);
        f[0] = hashed((uint32_t)bits(65, 12), 12); f[1] = hashed((uint32_t)bits(43, 22), 22); f[2] = buf;
        return true;
    }
    return false;
}
// the message's text (duplicate filter, ALL.TXT line): the reference's " ".join(msg_tuple) for i3 = 1, 2, 4; the empty fields of free
// text and telemetry are left out for the opt-in types
static std::string msg_line(uint64_t lo, const std::string f[3]) {
    const unsigned i3 = (unsigned)(lo & 7u);
    if (i3 == 0 || i3 == 3 || i3 == 5) return f[1].empty() ? f[0] : f[0] + " " + f[1] + " " + f[2];
    return f[0] + " " + f[1] + " " + f[2];
}
// the output row types of the packager: ft8rx_message (ft8rx_package_batch / _packed) and ft8rx_message_ext (ft8rx_package_batch_ext)
static void set_type(ft8rx_message&, uint64_t) {}
static void set_type(ft8rx_message_ext& o, uint64_t lo) { o.i3 = (uint8_t)(lo & 7u); o.n3 = o.i3 == 0 ? (uint8_t)((lo >> 3) & 7u) : 0; }
struct Ev { int cand, ipass, slot, seq; uint64_t lo, hi; };
static bool ev_before(const Ev& a, const Ev& b) {          // the reference's call order: candidate, ladder step, attempt, order inside it
    if (a.cand != b.cand) return a.cand < b.cand;
    if (a.ipass != b.ipass) return a.ipass < b.ipass;
    if (a.slot != b.slot) return a.slot < b.slot;
    return a.seq < b.seq;
}
// Capacity of this layer: the largest max_cands of either build (libft8rx_wide.so), so both copies package any record width the
// ABI allows.
enum { PKG_MAX_CANDS = 2048 };
static_assert(FT8RX_MAX_CANDS <= PKG_MAX_CANDS, "message layer capacity");
// -> number of messages written (<= cap).  *flags: FT8RX_PKG_MSG_TRUNCATED if more than cap messages were emitted.
// sparse = the records of a packed result buffer (include/ft8rx.h): only the candidates that decoded or logged an event, in candidate
// order, each carrying its candidate index in pad2.  The replay never looks at any other candidate, and a stable sort orders a
// subset exactly as it orders it inside the full list, so the messages are the ones the dense arrays give.
// mask: the opt-in message types (unpack_ext); 0 for ft8rx_message rows
template <typename Msg>
static int package_frame(const ft8rx_record* rec, int n, const ft8rx_event* ev, int nev, Msg* out, int cap, Hashes& H, int* flags,
                         bool sparse = false, unsigned mask = 0, const ft8rx_record* rrec = nullptr, int rn = 0) {
    std::vector<Ev> E; E.reserve((size_t)nev);
    int16_t pos[PKG_MAX_CANDS];
    if (sparse) {
        for (int i = 0; i < PKG_MAX_CANDS; i++) pos[i] = -1;
        for (int i = 0; i < n; i++) if (rec[i].pad2 < (uint32_t)PKG_MAX_CANDS) pos[rec[i].pad2] = (int16_t)i;
    }
    for (int i = 0; i < nev; i++) {
        int c = ev[i].cand;
        if (sparse) { c = c < PKG_MAX_CANDS ? pos[c] : -1; if (c < 0) continue; }
        E.push_back({c, ev[i].ipass, ev[i].slot, ev[i].seq, ev[i].msg_lo, ev[i].msg_hi});
    }
    std::sort(E.begin(), E.end(), ev_before);
    std::vector<int> last(n), order; order.reserve(n);
    for (int i = 0; i < n; i++) {
        const int st = rec[i].status;
        last[i] = st == FT8RX_ST_DECODED ? rec[i].ipass : st == FT8RX_ST_STOP_GRID_SD ? 0 : (st == FT8RX_ST_STOP_COSTAS || st == FT8RX_ST_STOP_FINE_SD) ? 1 : 7;
    }
    std::vector<std::string> seen; int nm = 0;
    for (int rnd = 0; rnd < 8; rnd++) {
        order.clear();
        for (int i = 0; i < n; i++) if (last[i] >= rnd) order.push_back(i);
        if (rnd == 1) std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rec[a].grid_sd > rec[b].grid_sd; });
        else if (rnd >= 2) std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rec[a].fine_sd > rec[b].fine_sd; });
        for (int i : order) {
            const ft8rx_record& r = rec[i];
            const bool here = r.status == FT8RX_ST_DECODED && r.ipass == rnd;
            int sslot = -1, sseq = -1;
            if (here) {
                const int m = r.method;
                sslot = rnd == 7 ? 2 * r.ap + (m == FT8RX_M_OSD ? 1 : 0) : r.ap + (m == FT8RX_M_LDPC_B_OSD ? 5 : 0);    // ipass 7: kernels/ap_calls.hpp
                sseq = m == FT8RX_M_GOOD91 ? 0 : (m == FT8RX_M_LDPC_A || m == FT8RX_M_LDPC_B) ? r.n_its + 1 : r.n_its;
            }
            std::string f[3], got[3]; bool have = false;
            Ev key{i, rnd, -1, -1, 0, 0};
            auto it = std::lower_bound(E.begin(), E.end(), key, ev_before);
            int pslot = -2, pseq = -2;
            for (; it != E.end() && it->cand == i && it->ipass == rnd; ++it) {
                if (here && (it->slot > sslot || (it->slot == sslot && it->seq > sseq))) break;
                if (it->slot == pslot && it->seq == pseq) continue;          // the same call logged twice
                pslot = it->slot; pseq = it->seq;
                const bool ok = unpack_ext(it->lo, it->hi, mask, H, f);
                if (here && it->slot == sslot && it->seq == sseq) { have = ok; if (ok) { got[0] = f[0]; got[1] = f[1]; got[2] = f[2]; } }
            }
            if (!here) continue;
            if (!have) { have = unpack_ext(r.msg_lo, r.msg_hi, mask, H, got); if (!have) continue; }    // event log truncated
            std::string text = msg_line(r.msg_lo, got);
            if (std::find(seen.begin(), seen.end(), text) != seen.end()) continue;
            seen.push_back(text);
            if (nm < cap) {
                Msg& o = out[nm]; memset(&o, 0, sizeof(o));
                const size_t W = sizeof(o.f[0]) - 1;
                for (int k = 0; k < 3; k++) { const size_t L = got[k].size() < W ? got[k].size() : W; memcpy(o.f[k], got[k].data(), L); }      // (o is zeroed: NUL-terminated)
                set_type(o, r.msg_lo);
                o.cand = (int16_t)(sparse ? (int)r.pad2 : i); o.f0_idx = r.f0_idx; o.h0_idx = r.h0_idx; o.ipass = r.ipass; o.ap = r.ap; o.method = r.method;
                const bool fine = rnd >= 2;
                o.fine = fine; o.snr = fine ? r.snr_fine : r.snr_grid; o.ttweak = fine ? r.ttweak : 0; o.ftweak = fine ? r.ftweak : 0;
            }
            nm++;
        }
    }
    // recall (ipass 8, ft8rx_fetch_recall): after every ladder message, in entry order; record e belongs to entry e (cand = e)
    for (int e = 0; e < rn; e++) {
        const ft8rx_record& r = rrec[e];
        if (r.ipass != 8 || r.status != FT8RX_ST_DECODED) continue;
        std::string got[3];
        if (!unpack_ext(r.msg_lo, r.msg_hi, mask, H, got)) continue;
        std::string text = msg_line(r.msg_lo, got);
        if (std::find(seen.begin(), seen.end(), text) != seen.end()) continue;
        seen.push_back(text);
        if (nm < cap) {
            Msg& o = out[nm]; memset(&o, 0, sizeof(o));
            const size_t W = sizeof(o.f[0]) - 1;
            for (int k = 0; k < 3; k++) { const size_t L = got[k].size() < W ? got[k].size() : W; memcpy(o.f[k], got[k].data(), L); }
            set_type(o, r.msg_lo);
            o.cand = (int16_t)e; o.f0_idx = r.f0_idx; o.h0_idx = r.h0_idx; o.ipass = r.ipass; o.ap = r.ap; o.method = r.method;
            o.fine = 1; o.snr = r.snr_fine; o.ttweak = r.ttweak; o.ftweak = r.ftweak;
        }
        nm++;
    }
    if (nm > cap) { if (flags) *flags |= FT8RX_PKG_MSG_TRUNCATED; nm = cap; }
    return nm;
}

// CRC-14 of a 77-bit message, bit-serial (decoders.py:123-129)
static inline unsigned crc14_serial(uint64_t lo, uint64_t hi) {
    unsigned r = 0;
    for (int i = 0; i < 96; i++) {
        unsigned b = 0;
        if (i < 77) { int pos = 76 - i; b = (unsigned)((pos >= 64 ? (hi >> (pos - 64)) : (lo >> pos)) & 1u); }
        unsigned top = (r >> 13) & 1u;
        r = ((r << 1) & 0x3FFFu) | b;
        if (top) r ^= 0x2757u;
    }
    return r;
}
// 77-bit word -> 79 tones (transmitter.py:181-223 encode_bits77): CRC-14, LDPC(174,91) systematic encode, Gray map, Costas framing
// 77-bit word -> 174-bit codeword: CRC-14, LDPC(174,91) systematic encode; codeword bit v at cw[v >> 6] bit v & 63
static void encode_cw174(uint64_t lo, uint64_t hi, uint64_t cw[3]) {
    hi &= 0x1FFFull;
    const unsigned crc = crc14_serial(lo, hi);
    cw[0] = cw[1] = cw[2] = 0;
    for (int r = 0; r < 91; r++) {                                 // message bit r: 77 message bits (bit 76 first), then the CRC
        unsigned b;
        if (r < 77) { const int pos = 76 - r; b = (unsigned)((pos >= 64 ? (hi >> (pos - 64)) : (lo >> pos)) & 1u); }
        else b = (crc >> (13 - (r - 77))) & 1u;
        if (b) { cw[0] ^= FT8_G0[r][0]; cw[1] ^= FT8_G0[r][1]; cw[2] ^= FT8_G0[r][2]; }
    }
}
// standard callsign -> c28 (FT8 protocol, i3 = 1: the form pyft8_amd/synth.py pack_c28 packs), -1 for anything else: the tokens
// DE / QRZ / CQ, hashed or compound calls, lower case, blanks.  3..6 characters, letters and digits; the digit is the second or
// third character; after it up to three letters.
static long pack_c28_std(const char* call) {
    if (!call) return -1;
    const size_t n = strlen(call);
    if (n < 3 || n > 6) return -1;
    for (size_t i = 0; i < n; i++) { const char ch = call[i]; if (!((ch >= 'A' && ch <= 'Z') || (ch >= '0' && ch <= '9'))) return -1; }
    char c[7] = "      ";
    if (call[2] >= '0' && call[2] <= '9') memcpy(c, call, n);
    else { if (n > 5) return -1; c[0] = ' '; memcpy(c + 1, call, n); }
    static const char* A0 = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ", *A1 = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ", *A3 = " ABCDEFGHIJKLMNOPQRSTUVWXYZ";
    if (!(c[2] >= '0' && c[2] <= '9')) return -1;
    const char* p0 = strchr(A0, c[0]), *p1 = strchr(A1, c[1]);
    if (!p0 || !p1 || !c[1] || c[1] == ' ') return -1;
    long v = (long)(p0 - A0);
    v = v * 36 + (long)(p1 - A1);
    v = v * 10 + (c[2] - '0');
    bool blank = false;
    for (int i = 3; i < 6; i++) {
        const char* q = strchr(A3, c[i]);
        if (!q || !c[i]) return -1;
        if (c[i] == ' ') blank = true; else if (blank) return -1;          // letters after a blank: not a call
        v = v * 27 + (long)(q - A3);
    }
    return v + 2063592L + 4194304L;                                  // NTOKENS + MAX22
}
static void encode_tones(uint64_t lo, uint64_t hi, uint8_t* t) {
    static const uint8_t costas[7] = {3, 1, 4, 0, 6, 5, 2}, gray[8] = {0, 1, 3, 2, 5, 6, 4, 7};
    uint64_t cw[3];
    encode_cw174(lo, hi, cw);
    for (int k = 0; k < 7; k++) { t[k] = costas[k]; t[36 + k] = costas[k]; t[72 + k] = costas[k]; }
    for (int sidx = 0; sidx < 58; sidx++) {
        unsigned v = 0;
        for (int b = 0; b < 3; b++) { const int bit = 3 * sidx + b; v = (v << 1) | (unsigned)((cw[bit >> 6] >> (bit & 63)) & 1ull); }
        t[(sidx < 29 ? 7 : 14) + sidx] = gray[v];
    }
}
// 77-bit word -> the 105 FT4 tones (pyft8_amd/ft4.py tones105): the word XOR rvec through the same CRC-14 and LDPC encode, two bits
// per symbol through the Gray map 0 1 3 2, framed  R S4a D29 S4b D29 S4c D29 S4d R  (R = tone 0; b, c, d = a XOR 1, 2, 3)
static void encode_tones_ft4(uint64_t lo, uint64_t hi, uint8_t* t) {
    static const uint8_t gray[4] = {0, 1, 3, 2};
    uint64_t cw[3];
    encode_cw174(lo ^ 0xd13696114f2ab7c5ull, (hi ^ 0x94bull) & 0x1FFFull, cw);        // rvec, first transmitted bit = bit 76
    t[0] = 0; t[104] = 0;
    for (int b = 0; b < 4; b++) for (int s = 0; s < 4; s++) t[1 + 33 * b + s] = (uint8_t)(gray[s] ^ b);
    for (int i = 0; i < 87; i++) {
        const int b0 = 2 * i, b1 = 2 * i + 1;
        const unsigned v = (unsigned)(((cw[b0 >> 6] >> (b0 & 63)) & 1ull) << 1) | (unsigned)((cw[b1 >> 6] >> (b1 & 63)) & 1ull);
        t[(i < 29 ? 5 : i < 58 ? 9 : 13) + i] = gray[v];
    }
}

// records/events of n_frames frames -> messages; table == nullptr: a fresh hash table per frame (frames spread over n_threads
// threads); table != nullptr: frames in order on the caller's thread, all sharing (and updating) that table.
// mask: the opt-in message types (ft8rx_package_batch_ext; Msg = ft8rx_message_ext)
template <typename Msg>
static int package_batch(const ft8rx_record* records, const int32_t* counts, const ft8rx_event* events, const int32_t* event_counts,
                         int n_frames, int max_cands, Msg* out, int max_msgs, int32_t* out_counts, int n_threads,
                         Hashes* table, int32_t* flags, unsigned mask = 0, const ft8rx_record* recall = nullptr,
                         const int32_t* recall_counts = nullptr) {
    if (!records || !counts || !events || !event_counts || !out || !out_counts || n_frames < 1 || max_cands < 1 || max_msgs < 1) return -1;
    if (n_threads < 1 || table) n_threads = 1;
    if (n_threads > n_frames) n_threads = n_frames;
    std::atomic<int> next{0};                                     // frames are handed out one by one: they differ in length
    auto work = [&](int) {
        Hashes local;                                             // one table per worker, emptied for every frame
        for (int f = next.fetch_add(1, std::memory_order_relaxed); f < n_frames; f = next.fetch_add(1, std::memory_order_relaxed)) {
            int fl = 0;
            int nev = event_counts[f];
            if (nev > FT8RX_EVENT_CAP) { nev = FT8RX_EVENT_CAP; fl |= FT8RX_PKG_EVENTS_TRUNCATED; }
            if (nev < 0) nev = 0;
            int n = counts[f] < 0 ? 0 : (counts[f] > max_cands ? max_cands : counts[f]);
            if (!table) local.clear();
            out_counts[f] = package_frame(records + (size_t)f * max_cands, n, events + (size_t)f * FT8RX_EVENT_CAP, nev,
                                          out + (size_t)f * max_msgs, max_msgs, table ? *table : local, &fl, false, mask,
                                          recall ? recall + (size_t)f * FT8RX_RECALL_MAX : nullptr,
                                          recall ? (recall_counts[f] < 0 ? 0 : recall_counts[f] > FT8RX_RECALL_MAX ? FT8RX_RECALL_MAX : recall_counts[f]) : 0);
            if (flags) flags[f] = fl;
        }
    };
    HostPool::run(n_threads, work);
    return 0;
}
// The same from a packed result buffer (header | frame table | kept records | used events; include/ft8rx.h): frames
// [frame_lo, frame_lo + n_frames) -> out[n_frames][max_msgs].  Every offset is checked against `bytes` before it is followed.
static int package_packed(const void* packed, uint64_t bytes, int frame_lo, int n_frames, ft8rx_message* out, int max_msgs,
                          int32_t* out_counts, int n_threads, Hashes* table, int32_t* flags) {
    if (!packed || !out || !out_counts || n_frames < 1 || frame_lo < 0 || max_msgs < 1 || bytes < sizeof(ft8rx_packed_header)) return -1;
    ft8rx_packed_header hd; memcpy(&hd, packed, sizeof(hd));
    if (hd.magic != FT8RX_PACKED_MAGIC || hd.overflow || hd.bytes > bytes || hd.n_frames < 0 || hd.n_records < 0 || hd.n_events < 0 ||
        (int64_t)frame_lo + n_frames > hd.n_frames) return -1;
    if (hd.bytes != sizeof(hd) + (uint64_t)hd.n_frames * sizeof(ft8rx_packed_frame) + (uint64_t)hd.n_records * sizeof(ft8rx_record) +
                    (uint64_t)hd.n_events * sizeof(ft8rx_event)) return -1;
    const unsigned char* base = (const unsigned char*)packed;
    const ft8rx_packed_frame* tab = (const ft8rx_packed_frame*)(base + sizeof(hd));
    const ft8rx_record* recs = (const ft8rx_record*)(base + sizeof(hd) + (size_t)hd.n_frames * sizeof(ft8rx_packed_frame));
    const ft8rx_event* evs = (const ft8rx_event*)((const unsigned char*)recs + (size_t)hd.n_records * sizeof(ft8rx_record));
    for (int f = frame_lo; f < frame_lo + n_frames; f++) {
        const ft8rx_packed_frame& t = tab[f];
        const int ne = t.n_ev > FT8RX_EVENT_CAP ? FT8RX_EVENT_CAP : (t.n_ev < 0 ? 0 : t.n_ev);
        if (t.rec_off < 0 || t.ev_off < 0 || (int64_t)t.rec_off + t.n_rec > hd.n_records || (int64_t)t.ev_off + ne > hd.n_events ||
            t.n_rec > PKG_MAX_CANDS) return -1;
    }
    if (n_threads < 1 || table) n_threads = 1;
    if (n_threads > n_frames) n_threads = n_frames;
    std::atomic<int> next{0};
    auto work = [&](int) {
        Hashes local;
        for (int i = next.fetch_add(1, std::memory_order_relaxed); i < n_frames; i = next.fetch_add(1, std::memory_order_relaxed)) {
            const ft8rx_packed_frame& t = tab[frame_lo + i];
            int fl = 0, nev = t.n_ev < 0 ? 0 : t.n_ev;
            if (nev > FT8RX_EVENT_CAP) { nev = FT8RX_EVENT_CAP; fl |= FT8RX_PKG_EVENTS_TRUNCATED; }
            if (!table) local.clear();
            out_counts[i] = package_frame(recs + t.rec_off, t.n_rec, evs + t.ev_off, nev, out + (size_t)i * max_msgs, max_msgs,
                                          table ? *table : local, &fl, true);
            if (flags) flags[i] = fl;
        }
    };
    HostPool::run(n_threads, work);
    return 0;
}
// Multi-pass decoding (extension): append the messages of a later pass that are new for their frame.
// out[f][0 .. out_counts[f]) holds the messages so far; add[f][0 .. add_counts[f]) the later pass's; a message is new if its three
// text fields differ from every message the frame already has.  New ones are appended to out (pad[0] = pass_tag) and, untagged, to
// fresh[f] -- the list the next subtraction sweep works from.  drop_osd: ignore OSD decodes (ipass 5 / 6) of the later pass.
static void merge_messages(ft8rx_message* out, int32_t* out_counts, int max_out, const ft8rx_message* add, const int32_t* add_counts,
                           int max_add, int n_frames, int pass_tag, int drop_osd, ft8rx_message* fresh, int32_t* fresh_counts) {
    for (int f = 0; f < n_frames; f++) {
        ft8rx_message* o = out + (size_t)f * max_out;
        const ft8rx_message* a = add + (size_t)f * max_add;
        ft8rx_message* fr = fresh ? fresh + (size_t)f * max_add : nullptr;
        int n = out_counts[f] < 0 ? 0 : out_counts[f], nf = 0;
        const int na = add_counts[f] < max_add ? add_counts[f] : max_add;
        for (int i = 0; i < na; i++) {
            if (drop_osd && (a[i].method == FT8RX_M_OSD || a[i].method == FT8RX_M_LDPC_B_OSD)) continue;
            if (n >= max_out) break;
            bool seen = false;
            for (int j = 0; j < n && !seen; j++) seen = memcmp(o[j].f, a[i].f, sizeof(a[i].f)) == 0;
            if (seen) continue;
            o[n] = a[i]; o[n].pad[0] = (uint8_t)pass_tag; n++;
            if (fr) fr[nf] = a[i];
            nf++;
        }
        out_counts[f] = n;
        if (fresh_counts) fresh_counts[f] = nf;
    }
}
// Input of a subtraction sweep (multi-pass extension): every message of a frame with snr > min_snr, in emit order, as
// (tones of its codeword, the decoder's origin: fHz = 3.125 f0_idx (+ ftweak / 16), tsec = h0_idx / 25 (+ ttweak / 200) -- the values
// the message dict reports, receiver.py:166).  -> the largest per-frame count.
static int subtraction_list(const ft8rx_message* msgs, const int32_t* counts, int max_msgs, const ft8rx_record* records, int max_cands,
                            int n_frames, int min_snr, ft8rx_subsig* sigs, int max_sigs, int32_t* sig_counts) {
    int most = 0;
    for (int f = 0; f < n_frames; f++) {
        const ft8rx_message* m = msgs + (size_t)f * max_msgs;
        ft8rx_subsig* o = sigs + (size_t)f * max_sigs;
        int n = 0;
        const int nm = counts[f] < max_msgs ? counts[f] : max_msgs;
        for (int i = 0; i < nm && n < max_sigs; i++) {
            if ((int)m[i].snr <= min_snr || m[i].cand < 0 || m[i].cand >= max_cands) continue;
            const ft8rx_record& r = records[(size_t)f * max_cands + m[i].cand];
            memset(&o[n], 0, sizeof(o[n]));
            encode_tones(r.msg_lo, r.msg_hi, o[n].tones);
            o[n].fHz = 3.125 * (double)m[i].f0_idx + (m[i].fine ? (double)m[i].ftweak / 16.0 : 0.0);
            o[n].tsec = (double)m[i].h0_idx / 25.0 + (m[i].fine ? (double)m[i].ttweak / 200.0 : 0.0);
            n++;
        }
        sig_counts[f] = n;
        if (n > most) most = n;
    }
    return most;
}
// Input of an FT4 subtraction sweep: a frame's decoded records in emit order -- the BP decodes (ipass 4),
// then OSD's (ipass 5), each in score order as package_frame replays them -- every 77-bit word once, at its first occurrence, none
// of the words the frame already has (have_lo / have_hi [n_frames][max_have], NULL = none); start = 144 h0 + 36 ttweak,
// fq = 4 f0 + ftweak.  A record whose fq falls outside [0, 4608) is left out.  -> the largest per-frame count, or -1.
static int ft4_subtraction_list(const ft8rx_record* records, const int32_t* counts, int max_cands, int n_frames, const uint64_t* have_lo,
                                const uint64_t* have_hi, const int32_t* have_counts, int max_have, ft8rx_ft4_subsig* sigs, int max_sigs,
                                int32_t* sig_counts) {
    if (!records || !counts || !sigs || !sig_counts || max_cands < 1 || n_frames < 1 || max_sigs < 1) return -1;
    const bool have = have_lo && have_hi && have_counts && max_have > 0;
    int most = 0;
    std::vector<int> order;
    for (int f = 0; f < n_frames; f++) {
        const ft8rx_record* rec = records + (size_t)f * max_cands;
        ft8rx_ft4_subsig* o = sigs + (size_t)f * max_sigs;
        const int nc = counts[f] < 0 ? 0 : counts[f] > max_cands ? max_cands : counts[f];
        order.clear();
        for (int i = 0; i < nc; i++) if (rec[i].status == FT8RX_ST_DECODED && (rec[i].ipass == 4 || rec[i].ipass == 5)) order.push_back(i);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            return rec[a].ipass != rec[b].ipass ? rec[a].ipass < rec[b].ipass : rec[a].fine_sd > rec[b].fine_sd; });
        const int nh = !have ? 0 : have_counts[f] < 0 ? 0 : have_counts[f] > max_have ? max_have : have_counts[f];
        int n = 0;
        for (int i : order) {
            if (n >= max_sigs) break;
            const ft8rx_record& r = rec[i];
            const uint64_t lo = r.msg_lo, hi = r.msg_hi & 0x1FFFull;
            bool seen = false;
            for (int j = 0; j < nh && !seen; j++) seen = have_lo[(size_t)f * max_have + j] == lo && (have_hi[(size_t)f * max_have + j] & 0x1FFFull) == hi;
            if (seen) continue;
            const int fq = 4 * (int)r.f0_idx + (int)r.ftweak;
            if (fq < 0 || fq >= 4608) continue;
            ft8rx_ft4_subsig g; memset(&g, 0, sizeof(g));
            encode_tones_ft4(lo, hi, g.tones);
            bool twice = false;                                           // the same word again: the remnant of a strong signal
            for (int j = 0; j < n && !twice; j++) twice = memcmp(o[j].tones, g.tones, sizeof(g.tones)) == 0;
            if (twice) continue;
            g.start = 144 * (int)r.h0_idx + 36 * (int)r.ttweak; g.fq = fq;
            o[n++] = g;
        }
        sig_counts[f] = n;
        if (n > most) most = n;
    }
    return most;
}
}  // namespace hostmsg

#endif
