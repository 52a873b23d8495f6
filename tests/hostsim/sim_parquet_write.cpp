// parquet_write.hpp compiled for the host, unchanged: the header writer, its length, the rows' rules and the bounds, for
// tests/test_parquet_write_model.py — as a shared object for ctypes, or (SIM_MAIN) as a stand-alone program over a file of cases, the
// form the sanitizer build takes.
#include "../../cramjam_amd/csrc/parquet_write.hpp"

namespace {
// the 14 words of a header's fields: type, usize, csize, crc, has_crc, num_values, num_nulls, num_rows, encoding, def_enc, rep_enc,
// def_len, rep_len, is_compressed
constexpr int kWords = 14;
cj::PqFields fields_of(const long long* w) {
    cj::PqFields f{};
    f.type = (int32_t)w[0]; f.usize = (int32_t)w[1]; f.csize = (int32_t)w[2]; f.crc = (uint32_t)w[3]; f.has_crc = w[4] != 0;
    f.num_values = (int32_t)w[5]; f.num_nulls = (int32_t)w[6]; f.num_rows = (int32_t)w[7]; f.encoding = (int32_t)w[8]; f.def_enc = (int32_t)w[9];
    f.rep_enc = (int32_t)w[10]; f.def_len = (int32_t)w[11]; f.rep_len = (int32_t)w[12]; f.is_compressed = w[13] != 0;
    return f;
}
void words_of(const cj::PqFields& f, long long* w) {
    const long long v[kWords] = {f.type, f.usize, f.csize, f.crc, f.has_crc, f.num_values, f.num_nulls, f.num_rows, f.encoding, f.def_enc, f.rep_enc, f.def_len, f.rep_len, f.is_compressed};
    for (int k = 0; k < kWords; k++) w[k] = v[k];
}
}  // namespace

extern "C" {

unsigned sim_pqw_max_header() { return cj::kPqMaxHeader; }
unsigned sim_pqw_header_len(const long long* w) { return cj::pq_header_len(fields_of(w)); }
// exactly sim_pqw_header_len(w) bytes at dst
unsigned sim_pqw_write_header(const long long* w, unsigned char* dst) { return cj::pq_write_header(dst, fields_of(w)); }

// parquet_grammar.hpp's reader over a written header: its code; *used = the bytes it took; w = what it read (num_nulls is not the
// reader's: 0; outside V2 is_compressed reads as true)
long long sim_pqw_read_back(const unsigned char* in, unsigned long long n, long long* w, unsigned long long* used) {
    cj::PqReader r{in, (size_t)n, 0};
    cj::PqPage pg;
    const long long err = cj::pq_page_header(r, pg);
    cj::PqFields f{};
    f.type = pg.type; f.usize = pg.usize; f.csize = pg.csize; f.crc = pg.crc; f.has_crc = pg.has_crc; f.num_values = pg.num_values; f.num_rows = pg.num_rows;
    f.encoding = pg.encoding; f.def_enc = pg.def_enc; f.rep_enc = pg.rep_enc; f.def_len = pg.def_len; f.rep_len = pg.rep_len; f.is_compressed = pg.is_compressed;
    words_of(f, w);
    *used = r.pos;
    return err;
}

// a row of the pages query's table -> the fields the writer reads (csize, crc, is_compressed stay 0), or its code
long long sim_pqw_row_fields(const long long* row, long long* w) {
    int64_t r[cj::kPqPageWords];
    for (size_t k = 0; k < cj::kPqPageWords; k++) r[k] = row[k];
    cj::PqFields f;
    const long long err = cj::pq_row_fields(r, f);
    words_of(f, w);
    return err;
}

unsigned long long sim_pqw_slot_bound(int codec, unsigned long long v) { return cj::pq_slot_bound(codec, v); }
unsigned long long sim_pqw_chunk_bound(int codec, unsigned long long n, unsigned long long pages) { return cj::pq_chunk_bound(codec, n, pages); }

}

#ifdef SIM_MAIN
#include <cstdio>
#include <cstdlib>
#include <cstring>
// The file: u32 count, then per case 14 x i64 fields | u32 len | the expected header.  Every destination is a heap block of exactly
// len bytes — flush against the end of its allocation, so a store behind the header's length is the sanitizer's — and so is the block
// the reader reads the header back from.
int main(int argc, char** argv) {
    FILE* f = argc < 2 ? nullptr : fopen(argv[1], "rb");
    uint32_t count = 0, bad = 0;
    if (!f || fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < count; c++) {
        long long w[kWords], back[kWords];
        uint32_t len;
        if (fread(w, 8, kWords, f) != (size_t)kWords || fread(&len, 4, 1, f) != 1 || len == 0 || len > cj::kPqMaxHeader) return 2;
        uint8_t* want = (uint8_t*)malloc(len);
        uint8_t* dst = (uint8_t*)malloc(len);
        if (fread(want, 1, len, f) != len) return 2;
        bool ok = sim_pqw_header_len(w) == len;
        if (ok) ok = sim_pqw_write_header(w, dst) == len && memcmp(dst, want, len) == 0;
        unsigned long long used = 0;
        if (ok) ok = sim_pqw_read_back(dst, len, back, &used) == 0 && used == len;
        if (!ok) { bad++; printf("case %u: length %u against %u\n", c, sim_pqw_header_len(w), len); }
        free(want); free(dst);
    }
    fclose(f);
    printf("%u cases, %u bad\n", count, bad);
    return bad ? 1 : 0;
}
#endif
