// tests/host_walk/walk_host.cpp
// The message walker on the CPU: kernels/message_walk.h and kernels/list_read.h compiled for the
// host, unmodified, behind the two headers under stubs/, one "lane" at a time. The library
// (libwalk_host.so) is what tests/test_walk_fuzz.py compares with the Python models; the program
// (WALK_HOST_MAIN) reads the units and tables that tests/walk_fuzz.py writes, copies every unit
// into a heap block of exactly its length and walks it there, so that under AddressSanitizer a
// load outside a message is a report. DESIGN.md §2.13, §2.14 (testing).
//
// list_heads_kernel runs as it is. The few lines that read_fields_kernel and read_elements_kernel
// have around their mw_* calls are restated below, each block marked with the lines it follows
// (struct_read.h includes wave intrinsics for gather_kernel and is not compiled here). What this
// twin cannot show: the 256 lanes of a block side by side in the LDS columns, the window and
// fallback parent lookup of read_elements_kernel, and gather_kernel.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kernels/common.h"
#include "kernels/list_read.h"
#include "kernels/message_walk.h"

using namespace cpk;

// follows packed_kernels.hip: sr_fields
static SrFields sr_fields(const capnp_packed_field* fields, uint32_t n_fields) {
    SrFields fs{};
    for (uint32_t f = 0; f < n_fields; ++f) {
        fs.f[f] = fields[f];
        const capnp_packed_field& a = fields[f];
        bool same = f > 0 && a.path_len == fields[f - 1].path_len;
        for (uint32_t k = 0; same && k < a.path_len; ++k) same = a.path[k] == fields[f - 1].path[k];
        if (same) fs.same |= 1u << f;
    }
    return fs;
}

// the LDS of read_fields_kernel and read_elements_kernel (struct_read.h:32-33, list_read.h:237)
static uint32_t segb_all[(kSrSegs + 1) * kBlock];
static uint32_t res_all[4 * kSrGroup * kBlock];

extern "C" {

// read_fields_kernel for units [0, n): unit i runs as thread i % 256, so every LDS column is used
void walk_read_fields(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                      const capnp_packed_field* fields, uint32_t n_fields, uint64_t* value, uint64_t* flen,
                      uint64_t* count, int32_t* status) {
    if (n_fields == 0) return;
    const SrFields fs = sr_fields(fields, n_fields);
    for (uint32_t i = 0; i < n; ++i) {
        threadIdx.x = i % kBlock;
        blockIdx.x = i / kBlock;
        // ---- follows struct_read.h:34-47 (read_fields_kernel's body) ----------------------------
        const uint32_t msg = blockIdx.x * kBlock + threadIdx.x;
        const uint64_t moff = in_off[msg];
        const uint64_t len = in_len[msg];
        const uint8_t* const d = in + moff;
        const MwStage out{res_all + threadIdx.x, msg, n, value, flen, count, status};
        auto fail_all = [&](int32_t st) { out.store_all(n_fields, st); };

        uint32_t nseg;
        if (int32_t st = mw_init(d, moff, len, segb_all + threadIdx.x, nseg)) { fail_all(st); continue; }
        MwSegsLds sg{d, nseg, segb_all + threadIdx.x};
        MwStruct root{};
        if (int32_t st = mw_root(sg, root)) { fail_all(st); continue; }
        mw_read_fields(sg, moff, root, fs, n_fields, out);
        // ---- end ----------------------------------------------------------------------------------
    }
}

// list_heads_kernel itself, one lane a call
void walk_list_heads(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                     const uint32_t* path, uint32_t path_len, uint32_t pointer_index, uint32_t list_kind,
                     capnp_packed_list_head* head, uint64_t* count, int32_t* status) {
    LrPath p{};  // follows packed_kernels.hip: launch_list_heads
    for (uint32_t k = 0; k < path_len; ++k) p.p[k] = path[k];
    for (uint32_t i = 0; i < n; ++i) {
        threadIdx.x = i % kBlock;
        blockIdx.x = i / kBlock;
        list_heads_kernel(in, in_off, in_len, n, p, path_len, pointer_index, list_kind, head, count, status);
    }
}

// read_elements_kernel for elements [0, min(start[n], elem_cap)): element e runs as thread e % 256.
// The parent comes from a bisection of the whole of `start`, which is the kernel's fallback
// (list_read.h:262-264); its LDS window is the device test's.
void walk_read_elements(const uint8_t* in, const uint64_t* in_off, uint32_t n, const capnp_packed_list_head* head,
                        const uint64_t* start, uint32_t list_kind, uint64_t elem_cap,
                        const capnp_packed_field* fields, uint32_t n_fields, uint32_t* parent, uint32_t* index,
                        uint64_t* value, uint64_t* flen, uint64_t* count, int32_t* status) {
    const SrFields fs = sr_fields(fields, n_fields);
    const uint64_t total = start[n] < elem_cap ? start[n] : elem_cap;
    for (uint64_t e = 0; e < total; ++e) {
        threadIdx.x = (uint32_t)(e % kBlock);
        blockIdx.x = (uint32_t)(e / kBlock);
        const uint32_t ub = lr_upper_bound(start, n, e);
        const uint32_t msg = ub ? ub - 1 : 0;
        const uint64_t first = start[msg];
        // ---- follows list_read.h:266-294 (read_elements_kernel after the parent lookup) ----------
        const uint64_t k = e - first;
        const MwStage out{res_all + threadIdx.x, e, elem_cap, value, flen, count, status};
        auto numbering = [&]() {
            if (parent) parent[e] = msg;
            if (index) index[e] = (uint32_t)k;
        };
        if (n_fields == 0) { numbering(); continue; }

        const capnp_packed_list_head h = head[msg];
        if (k >= h.count) {
            out.store_all(n_fields, ST_ARG);
            numbering();
            continue;
        }
        const uint64_t moff = in_off[msg];
        MwSegsHead sg{in + moff, h.segment, h.seg_begin, h.seg_bytes, 0};
        MwStruct elem{h.segment, h.seg_begin, h.elems_off - moff - h.seg_begin, 0, 1};
        if (list_kind == CAPNP_PACKED_LIST_STRUCT) {
            elem.dw = h.data_words;
            elem.pc = h.pointer_words;
            elem.off += k * 8ull * ((uint32_t)h.data_words + h.pointer_words);
        } else {
            elem.off += 8ull * k;
        }

        mw_read_fields(sg, moff, elem, fs, n_fields, out);
        numbering();
        // ---- end ----------------------------------------------------------------------------------
    }
}

}  // extern "C"

#ifdef WALK_HOST_MAIN
// walk_fuzz_main UNITS TABLES OUT: read_fields with the first table and every list run of TABLES
// over every unit of UNITS, each unit in a heap block of exactly its length. OUT, all uint64:
//   per unit, per field: status, value, len, count
//   per run: per unit the 32-byte head; then per unit: rows, and per row and field status, value,
//   len, count (at most `limit` rows of a list)
// Slice values and elems_off are written as offsets in the unit. Prints the status histograms.
namespace {

struct Reader {
    std::vector<uint8_t> raw;
    size_t at = 0;
    explicit Reader(const char* path) {
        FILE* f = fopen(path, "rb");
        if (!f) { perror(path); exit(2); }
        uint8_t buf[1 << 16];
        for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + k);
        fclose(f);
    }
    uint32_t u32() {
        uint32_t v;
        take(&v, 4);
        return v;
    }
    void take(void* to, size_t k) {
        if (at + k > raw.size()) { fprintf(stderr, "walk_fuzz: input file too short\n"); exit(2); }
        if (k) memcpy(to, raw.data() + at, k);
        at += k;
    }
    std::vector<capnp_packed_field> fields() {
        std::vector<capnp_packed_field> f(u32());
        if (f.size() > CAPNP_PACKED_MAX_FIELDS) { fprintf(stderr, "walk_fuzz: more than 32 fields\n"); exit(2); }
        take(f.data(), f.size() * sizeof(capnp_packed_field));
        return f;
    }
};

struct Run {
    uint32_t kind, index, path_len, path[CAPNP_PACKED_MAX_PATH];
    std::vector<capnp_packed_field> fields;
};

void put(FILE* f, const void* p, size_t k) {
    if (k && fwrite(p, 1, k, f) != k) { perror("write"); exit(2); }
}

void histogram(const char* what, const uint64_t (&h)[32]) {
    printf("%s:", what);
    for (int s = 0; s < 32; ++s)
        if (h[s]) printf(" %d=%llu", s, (unsigned long long)h[s]);
    printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s UNITS TABLES OUT\n", argv[0]); return 2; }
    Reader units(argv[1]), tables(argv[2]);
    FILE* const fo = fopen(argv[3], "wb");
    if (!fo) { perror(argv[3]); return 2; }

    // every unit in a block of its own, of exactly its length; offsets count from the lowest block
    const uint32_t n = units.u32();
    std::vector<uint8_t*> block(n);
    std::vector<uint64_t> off(n), len(n);
    uintptr_t lowest = UINTPTR_MAX;
    for (uint32_t i = 0; i < n; ++i) {
        len[i] = units.u32();
        block[i] = static_cast<uint8_t*>(malloc(len[i]));
        if (!block[i]) block[i] = static_cast<uint8_t*>(malloc(1));
        units.take(block[i], len[i]);
        if (reinterpret_cast<uintptr_t>(block[i]) < lowest) lowest = reinterpret_cast<uintptr_t>(block[i]);
    }
    const uint8_t* const in = reinterpret_cast<const uint8_t*>(lowest);
    for (uint32_t i = 0; i < n; ++i) off[i] = reinterpret_cast<uintptr_t>(block[i]) - lowest;

    uint64_t h_field[32] = {}, h_head[32] = {}, h_elem[32] = {};
    // a slice's value as an offset in its unit (a data kind's value and the 0 of a failed or empty read stay)
    auto record = [&](const capnp_packed_field& F, uint64_t moff, int32_t st, uint64_t v, uint64_t l, uint64_t c,
                      uint64_t (&h)[32]) {
        ++h[st & 31];
        if (F.kind > CAPNP_PACKED_FIELD_BOOL && st == ST_OK && v) v -= moff;
        const uint64_t rec[4] = {(uint64_t)(int64_t)st, v, l, c};
        put(fo, rec, sizeof rec);
    };

    {   // ---- read_fields ------------------------------------------------------------------------
        const std::vector<capnp_packed_field> fields = tables.fields();
        const size_t nf = fields.size(), cells = nf * n;
        std::vector<uint64_t> value(cells, ~0ull), flen(cells, ~0ull), count(cells, ~0ull);
        std::vector<int32_t> status(cells, -1);
        walk_read_fields(in, off.data(), len.data(), n, fields.data(), (uint32_t)nf, value.data(), flen.data(),
                         count.data(), status.data());
        for (uint32_t i = 0; i < n; ++i)
            for (size_t f = 0; f < nf; ++f)
                record(fields[f], off[i], status[f * n + i], value[f * n + i], flen[f * n + i], count[f * n + i], h_field);
    }
    const uint32_t n_runs = tables.u32(), limit = tables.u32();
    uint64_t elements = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {  // ---- heads -> a scan of the counts -> elements ---------
        Run run;
        run.kind = tables.u32(), run.index = tables.u32(), run.path_len = tables.u32();
        for (uint32_t& p : run.path) p = tables.u32();
        run.fields = tables.fields();
        const size_t nf = run.fields.size();
        std::vector<capnp_packed_list_head> head(n);
        std::vector<uint64_t> hcount(n, ~0ull), start(n + 1, 0);
        std::vector<int32_t> hstatus(n, -1);
        memset(head.data(), 0xA5, n * sizeof(capnp_packed_list_head));
        walk_list_heads(in, off.data(), len.data(), n, run.path, run.path_len, run.index, run.kind, head.data(),
                        hcount.data(), hstatus.data());
        for (uint32_t i = 0; i < n; ++i) {
            ++h_head[hstatus[i] & 31];
            if (hstatus[i] != head[i].status || hcount[i] != head[i].count) {
                fprintf(stderr, "walk_fuzz: unit %u: the head, the count and the status disagree\n", i);
                return 1;
            }
            capnp_packed_list_head h = head[i];
            if (h.status == ST_OK) h.elems_off -= off[i];
            put(fo, &h, sizeof h);
            start[i + 1] = start[i] + (h.count < limit ? h.count : limit);  // an untrusted count: bounded here
        }
        const uint64_t total = start[n], cells = nf * total;
        elements += total;
        std::vector<uint64_t> value(cells, ~0ull), flen(cells, ~0ull), count(cells, ~0ull);
        std::vector<int32_t> status(cells, -1);
        std::vector<uint32_t> parent(total, ~0u), index(total, ~0u);
        walk_read_elements(in, off.data(), n, head.data(), start.data(), run.kind, total, run.fields.data(),
                           (uint32_t)nf, parent.data(), index.data(), value.data(), flen.data(), count.data(),
                           status.data());
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t rows = start[i + 1] - start[i];
            put(fo, &rows, sizeof rows);
            for (uint64_t e = start[i]; e < start[i + 1]; ++e) {
                if (parent[e] != i || index[e] != e - start[i]) {
                    fprintf(stderr, "walk_fuzz: element %llu: wrong parent or index\n", (unsigned long long)e);
                    return 1;
                }
                for (size_t f = 0; f < nf; ++f)
                    record(run.fields[f], off[i], status[f * total + e], value[f * total + e], flen[f * total + e],
                           count[f * total + e], h_elem);
            }
        }
    }
    if (fclose(fo)) { perror("close"); return 2; }
    for (uint8_t* b : block) free(b);
    printf("walk_fuzz: %u units, %u list runs, %llu elements\n", n, n_runs, (unsigned long long)elements);
    histogram("field statuses", h_field);
    histogram("head statuses", h_head);
    histogram("element statuses", h_elem);
    return 0;
}
#endif
