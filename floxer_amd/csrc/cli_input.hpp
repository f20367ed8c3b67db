// The CLI's inputs: FASTA / FASTQ (plain or gz, input.cpp:36-148) and the device list.
#pragma once
#include <zlib.h>

#include <chrono>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

struct LineReader {
    gzFile f;
    std::vector<char> buf;
    explicit LineReader(const char* path);
    ~LineReader();
    bool getline(std::string& out);
};

struct Reference { std::vector<std::string> ids; std::vector<uint64_t> lens; std::vector<uint8_t> pool; };

bool read_references(std::string const& path, Reference& ref, std::string& err);

// ---------------------------------------------------------------- FASTQ, block-parallel (input.cpp:83-148)
// The file is read (and, for .gz, inflated: one gzip stream is serial) in blocks by the calling thread; everything after that is
// parallel over the records of a batch: line boundaries, ids, rank encoding. A batch keeps its raw text: ids and qualities are
// pointers into it (terminated in place), so nothing is copied per record.
unsigned io_threads(uint64_t cli_threads);

// std::vector<char> value-initialises what resize() adds: 16 MB of zeroes in front of every 16-MB read. This allocator leaves it alone.
template <class T>
struct DefaultInit : std::allocator<T> {
    template <class U> struct rebind { using other = DefaultInit<U>; };
    template <class U> void construct(U* p) noexcept(std::is_nothrow_default_constructible<U>::value) { ::new (static_cast<void*>(p)) U; }
    template <class U, class... A> void construct(U* p, A&&... a) { ::new (static_cast<void*>(p)) U(std::forward<A>(a)...); }
};

struct ReadBatch {
    std::vector<char, DefaultInit<char>> raw;   // the batch's FASTQ text; ids / quals point into it
    std::vector<size_t> nl;                     // line ends of the text (FastqReader::next_text), four per record
    size_t n_rec = 0;                           // records the text holds
    std::vector<const char*> ids, quals;
    std::vector<uint8_t> pool;
    std::vector<uint64_t> offsets{0};
    size_t size() const { return ids.size(); }
};

struct FastqReader {
    gzFile f = nullptr;                         // gzip input
    int fd = -1;                                // plain input: read() straight into the batch's text (zlib's transparent mode copies every byte twice more)
    std::vector<char, DefaultInit<char>> carry; // text behind the last complete record of the previous batch
    bool eof = false;
    unsigned threads;
    size_t file_pos = 0, last_batch_bytes = 0;  // plain input: where the next read starts; the text the last batch took
    double s_read = 0, s_scan = 0, s_records = 0; // seconds spent reading, finding line ends, and on the records (FLX_CLI_PROFILE)
    static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    FastqReader(const char* path, unsigned threads_);
    ~FastqReader();
    bool is_open() const { return f != nullptr || fd >= 0; }

    // the next batch of up to max_reads records; false at the end of the file or on a malformed record (err set)
    bool next(ReadBatch& b, size_t max_reads, std::string& err);
    // Stage one, the reader's own thread: the text of the next batch (whole records) and its line ends. Stage two (parse_records) needs
    // nothing but the batch: the CLI runs it in the batch's task, next to the other batches' alignment, so that the one thread that has to
    // read the file in order does nothing else (it was the bound of the CLI with -I: 2.9 of 3.4 s).
    bool next_text(ReadBatch& b, size_t max_reads, std::string& err);
    // Stage two: ids, sequences (rank-encoded into the batch's pool) and qualities of the batch's records; false on a malformed record
    static bool parse_records(ReadBatch& b, unsigned threads, std::string& err);
};

// The devices of a list ("0", "0-7", "0,2,4", "all"); an empty spec means FLX_DEVICES, then FLX_DEVICE, then device 0
std::vector<int> parse_devices(std::string spec, int n_available, std::string& err);
