#include "cli_input.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "../../include/floxer_amd.h"
#include "cli_log.hpp"

LineReader::LineReader(const char* path) : f(gzopen(path, "rb")), buf(1 << 16) { if (f) gzbuffer(f, 1 << 20); }
LineReader::~LineReader() { if (f) gzclose(f); }
bool LineReader::getline(std::string& out) {
    out.clear();
    while (true) {
        if (!gzgets(f, buf.data(), (int)buf.size())) return !out.empty();
        size_t const n = strlen(buf.data());
        out.append(buf.data(), n);
        if (n && out.back() == '\n') { out.pop_back(); if (!out.empty() && out.back() == '\r') out.pop_back(); return true; }
    }
}

static std::string record_id(std::string const& tag) { return tag.substr(0, tag.find(' ')); }     // input.cpp:161-163

bool read_references(std::string const& path, Reference& ref, std::string& err) {
    LineReader in(path.c_str());
    if (!in.f) { err = "cannot open " + path; return false; }
    std::string line, id, seq;
    bool have = false;
    auto flush = [&]() {
        if (!have) return;
        if (seq.empty()) { log_line("warning", "The record %s in the reference file has an empty sequence and will be skipped.", id.c_str()); return; }
        ref.ids.push_back(id);
        ref.lens.push_back(seq.size());
        size_t const off = ref.pool.size();
        ref.pool.resize(off + seq.size());
        flx_chars_to_rank_sequence(seq.data(), seq.size(), ref.pool.data() + off);
        log_line("debug", "read reference, id: %s, length %zu", id.c_str(), seq.size());
    };
    while (in.getline(line)) {
        if (!line.empty() && line[0] == '>') { flush(); id = record_id(line.substr(1)); seq.clear(); have = true; }
        else if (have) seq += line;
    }
    flush();
    if (ref.ids.empty()) { err = "The reference file is empty, which is not allowed."; return false; }
    return true;
}

unsigned io_threads(uint64_t cli_threads) {
    if (const char* env = getenv("FLX_IO_THREADS")) { unsigned const v = (unsigned)strtoul(env, nullptr, 10); if (v) return std::min(v, 64u); }
    unsigned const hw = std::max(1u, std::thread::hardware_concurrency());
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(cli_threads, std::min(hw, 8u)), 64));
}
template <class F>
static void parallel_for(size_t n, unsigned threads, F&& body) {      // body(first, last) on disjoint ranges
    unsigned const t = (unsigned)std::min<size_t>(threads, std::max<size_t>(1, n / 256));
    if (t <= 1) { body((size_t)0, n); return; }
    std::vector<std::thread> pool;
    for (unsigned i = 0; i < t; ++i) pool.emplace_back([&, i] { body(n * i / t, n * (i + 1) / t); });
    for (auto& th : pool) th.join();
}

FastqReader::FastqReader(const char* path, unsigned threads_) : threads(threads_) {
    int const probe = open(path, O_RDONLY);
    if (probe < 0) return;
    // the pread path needs a file that can be read at an offset; a FIFO, /dev/stdin or a socket (plain or gzip: the reference reads a
    // pipe named *.fastq through an ifstream just as well) goes through zlib, whose transparent mode passes plain text through
    struct stat st;
    if (fstat(probe, &st) != 0 || !S_ISREG(st.st_mode)) {
        f = gzdopen(probe, "rb");
        if (f) gzbuffer(f, 1 << 20); else close(probe);
        return;
    }
    unsigned char magic[2] = {0, 0};
    ssize_t const got = pread(probe, magic, 2, 0);
    if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
        close(probe);
        f = gzopen(path, "rb");
        if (f) gzbuffer(f, 1 << 20);
    } else fd = probe;
}
FastqReader::~FastqReader() { if (f) gzclose(f); if (fd >= 0) close(fd); }

bool FastqReader::next(ReadBatch& b, size_t max_reads, std::string& err) {
    if (!next_text(b, max_reads, err)) return false;
    double const t_records = now_s();
    bool const ok = parse_records(b, threads, err);
    s_records += now_s() - t_records;
    return ok;
}

bool FastqReader::next_text(ReadBatch& b, size_t max_reads, std::string& err) {
    // (a recycled batch keeps its buffers: 330 MB of text and 165 MB of ranks per 16384 reads of 10 kb are not faulted in again)
    b.ids.clear(); b.quals.clear(); b.pool.clear(); b.offsets.assign(1, 0);
    auto& raw = b.raw;
    raw.clear();
    raw.insert(raw.end(), carry.begin(), carry.end());
    carry.clear();
    // ---- read until the text holds max_reads records (4 lines each) or the file ends
    size_t lines = 0, scanned = 0;
    std::vector<size_t>& nl = b.nl;         // positions of the line ends
    nl.clear();
    b.n_rec = 0;
    auto scan = [&]() {                     // line ends of raw[scanned, size): pieces of at least 8 MB, one thread each
        double const t_scan = now_s();
        size_t const lo = scanned, hi = raw.size();
        unsigned const t = (unsigned)std::min<size_t>(std::max(1u, threads), std::max<size_t>(1, (hi - lo) >> 23));
        std::vector<std::vector<size_t>> found(t);
        auto piece = [&](unsigned i) {
            size_t at = lo + (hi - lo) * i / t;
            size_t const end = lo + (hi - lo) * (i + 1) / t;
            while (at < end) {
                const char* p = (const char*)memchr(raw.data() + at, '\n', end - at);
                if (!p) break;
                found[i].push_back((size_t)(p - raw.data()));
                at = (size_t)(p - raw.data()) + 1;
            }
        };
        std::vector<std::thread> pool;
        for (unsigned i = 1; i < t; ++i) pool.emplace_back(piece, i);
        piece(0);
        for (auto& th : pool) th.join();
        for (auto const& v : found) { nl.insert(nl.end(), v.begin(), v.end()); lines += v.size(); }
        scanned = hi;
        s_scan += now_s() - t_scan;
    };
    scan();
    while (!eof && lines < 4 * max_reads) {
        // plain input: as much as the last batch took (and a little more) in one go, the pieces read by several threads (pread);
        // gzip input: 16 MB at a time through zlib
        size_t const at = raw.size(), want = f ? (size_t)16 << 20 : std::max<size_t>((size_t)16 << 20, last_batch_bytes > at ? last_batch_bytes - at + (1u << 20) : (size_t)16 << 20);
        double const t_read = now_s();
        raw.resize(at + want);
        long got;
        if (f) got = gzread(f, raw.data() + at, (unsigned)want);
        else {
            unsigned const t = (unsigned)std::min<size_t>(std::max(1u, threads), std::max<size_t>(1, want >> 24));      // >= 16 MB per thread
            std::vector<long> part(t, 0);
            std::vector<std::thread> pool;
            auto piece = [&](unsigned i) {
                size_t const lo = want * i / t, hi = want * (i + 1) / t;
                size_t done = 0;
                while (lo + done < hi) {
                    ssize_t const r = pread(fd, raw.data() + at + lo + done, hi - lo - done, (off_t)(file_pos + lo + done));
                    if (r < 0) { if (errno == EINTR) continue; part[i] = -1; return; }
                    if (r == 0) break;
                    done += (size_t)r;
                }
                part[i] = (long)done;
            };
            for (unsigned i = 1; i < t; ++i) pool.emplace_back(piece, i);
            piece(0);
            for (auto& th : pool) th.join();
            got = 0;
            for (unsigned i = 0; i < t && got >= 0; ++i) {
                if (part[i] < 0) got = -1;
                else { got += part[i]; if ((size_t)part[i] < want * (i + 1) / t - want * i / t) break; }      // a short piece: the file ends inside it
            }
            if (got > 0) file_pos += (size_t)got;
        }
        if (got < 0) { err = "read error on the query file"; return false; }
        raw.resize(at + (size_t)got);
        s_read += now_s() - t_read;
        if (f && (size_t)got < want) {
            // a short read is the end of the data only when zlib agrees (a truncated .gz ends with Z_BUF_ERROR / Z_DATA_ERROR)
            int zerr = Z_OK;
            (void)gzerror(f, &zerr);
            if (zerr != Z_OK && zerr != Z_STREAM_END) { err = "the query file is truncated or corrupt (gzip stream error)"; return false; }
            eof = true;
        }
        if (!f && got == 0) eof = true;
        scan();
    }
    if (eof && !raw.empty() && raw.back() != '\n') { nl.push_back(raw.size()); raw.push_back('\n'); ++lines; }   // last line without a line end
    // blank lines at the very end of the file are not records
    while (eof && lines % 4 != 0 && lines > 0 && nl.size() >= 1 && (lines == 1 ? nl[0] == 0 : nl[lines - 1] == nl[lines - 2] + 1)) { nl.pop_back(); --lines; }
    size_t n_rec = std::min(lines / 4, max_reads);
    if (eof && lines % 4 != 0 && lines / 4 < max_reads) { err = "truncated FASTQ record at the end of the query file"; return false; }
    size_t const used = n_rec ? nl[4 * n_rec - 1] + 1 : 0;
    carry.assign(raw.begin() + (long)used, raw.end());
    raw.resize(used);
    last_batch_bytes = used;
    if (n_rec == 0) return false;
    b.n_rec = n_rec;
    return true;
}

bool FastqReader::parse_records(ReadBatch& b, unsigned threads, std::string& err) {
    auto& raw = b.raw;
    std::vector<size_t> const& nl = b.nl;
    size_t const n_rec = b.n_rec;
    // ---- records: id (up to the first blank, input.cpp:161-163), sequence, quality; terminated in place
    struct Rec { size_t id, seq, seq_len, qual; bool keep; };
    std::vector<Rec> recs(n_rec);
    std::atomic<bool> bad{false}, bad_qual{false};
    parallel_for(n_rec, threads, [&](size_t r0, size_t r1) {
        for (size_t r = r0; r < r1; ++r) {
            size_t const l0 = r ? nl[4 * r - 1] + 1 : 0, e0 = nl[4 * r], l1 = e0 + 1, e1 = nl[4 * r + 1], l3 = nl[4 * r + 2] + 1, e3 = nl[4 * r + 3];
            if (raw[l0] != '@' || raw[nl[4 * r + 1] + 1] != '+') { bad = true; continue; }
            size_t id_end = e0;
            if (id_end > l0 && raw[id_end - 1] == '\r') --id_end;
            for (size_t i = l0 + 1; i < id_end; ++i) if (raw[i] == ' ') { id_end = i; break; }
            raw[id_end] = 0;
            size_t s_end = e1, q_end = e3;
            if (s_end > l1 && raw[s_end - 1] == '\r') --s_end;
            if (q_end > l3 && raw[q_end - 1] == '\r') --q_end;
            raw[q_end] = 0;
            if (q_end - l3 != s_end - l1) { bad_qual = true; continue; }             // input.cpp:137 asserts qual.size() == seq.size()
            recs[r] = Rec{l0 + 1, l1, s_end - l1, l3, true};
        }
    });
    if (bad) { err = "malformed FASTQ record in the query file"; return false; }
    if (bad_qual) { err = "a FASTQ record's sequence and quality differ in length"; return false; }
    for (auto& rc : recs) {                 // the reference's filters on the way in (input.cpp:95-110)
        if (rc.seq_len == 0) { log_line("warning", "The record %s in the query file has an empty sequence and will be skipped.", raw.data() + rc.id); rc.keep = false; }
        else if (rc.seq_len > 100000) { log_line("warning", "skipping too large query: %s", raw.data() + rc.id); rc.keep = false; }
    }
    recs.erase(std::remove_if(recs.begin(), recs.end(), [](Rec const& x) { return !x.keep; }), recs.end());
    b.ids.resize(recs.size());
    b.quals.resize(recs.size());
    b.offsets.assign(recs.size() + 1, 0);
    for (size_t r = 0; r < recs.size(); ++r) b.offsets[r + 1] = b.offsets[r] + recs[r].seq_len;
    b.pool.resize(b.offsets.back() + 1);
    parallel_for(recs.size(), threads, [&](size_t r0, size_t r1) {
        for (size_t r = r0; r < r1; ++r) {
            b.ids[r] = raw.data() + recs[r].id;
            b.quals[r] = raw.data() + recs[r].qual;
            flx_chars_to_rank_sequence(raw.data() + recs[r].seq, recs[r].seq_len, b.pool.data() + b.offsets[r]);
        }
    });
    return true;
}

std::vector<int> parse_devices(std::string spec, int n_available, std::string& err) {
    std::vector<int> out;
    if (spec.empty()) if (const char* env = getenv("FLX_DEVICES")) spec = env;
    if (spec.empty()) { if (const char* env = getenv("FLX_DEVICE")) spec = env; }
    if (spec.empty()) return {0};
    if (spec == "all") { for (int d = 0; d < n_available; ++d) out.push_back(d); return out; }
    size_t at = 0;
    while (at <= spec.size()) {
        size_t const comma = spec.find(',', at);
        std::string const part = spec.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        size_t const dash = part.find('-');
        char* end = nullptr;
        long const lo = strtol(part.c_str(), &end, 10);
        long hi = lo;
        if (dash != std::string::npos) hi = strtol(part.c_str() + dash + 1, &end, 10);
        if (part.empty() || *end || lo < 0 || hi < lo) { err = "cannot parse the device list " + spec; return {}; }
        for (long d = lo; d <= hi; ++d) out.push_back((int)d);
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    for (int d : out) if (d >= n_available) { err = "device " + std::to_string(d) + " of the device list does not exist (" + std::to_string(n_available) + " HIP devices)"; return {}; }
    return out;
}
