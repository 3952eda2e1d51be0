// FastqStorage.h — reads the FASTQ inputs and owns the reads (reference src/FastqStorage.h:25-107,
// src/FastqStorage.cpp:38-235).  Same public members the hot path uses: m_read_vec (singles
// first, then pairs), m_ID_to_index, m_readcount_single/_paired.  Storage is flat: one byte
// arena for bases, one for qualities, offsets per sequence — exactly what hc_set_reads takes.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "DefaultInit.h"
#include "Read.h"
#include "Types.h"

namespace hc {

// The flat base / quality arrays: bytes that resize() adds are left uninitialised (DefaultInit.h)
using ByteVec = std::vector<uint8_t, DefaultInitAllocator<uint8_t>>;

class FastqStorage {
public:
    explicit FastqStorage(const ProgramSettings& ps);

    std::vector<Read> m_singles_vec;
    std::vector<Read> m_paired_vec;
    std::vector<Read*> m_read_vec;                       // singles first, then pairs
    std::map<read_id_t, unsigned int> m_ID_to_index;    // first occurrence of an id wins (std::map::insert)
    unsigned int m_readcount_single = 0;
    unsigned int m_readcount_paired = 0;
    unsigned int m_largest_read_id = 0;

    Read* get_read(read_id_t ID);                        // src/FastqStorage.cpp:33-36
    unsigned int get_readcount() const { return (unsigned int)m_read_vec.size(); }

    // flat layout (hc_set_reads arguments)
    const ByteVec& bases() const { if (m_lazy_bytes) fill_bytes(); return m_bases; }
    const ByteVec& quals() const { if (m_lazy_bytes) fill_bytes(); return m_quals; }
    const std::vector<uint64_t>& seq_off() const { return m_seq_off; }
    const std::vector<uint32_t>& read_first_seq() const { return m_first; }
    // sequence index of mate i (0 = single, 1 = /1, 2 = /2) of read `index`
    uint32_t seq_index(unsigned int index, int i) const { return m_first[index] + (i == 2 ? 1u : 0u); }
    uint32_t seq_len(uint32_t q) const { return (uint32_t)(m_seq_off[q + 1] - m_seq_off[q]); }

    // The id side of the readers on its own, for the device reader (hc_api_fastq.cpp: hc_set_reads_from_fastq_text): a storage that holds
    // the --IDs map and nothing else (ids_path empty: no map), the header's token as `stream >> id` takes it, an id from a token, and one
    // record's checks in the readers' order with the readers' messages (l2 / n2 are read for a pair only).  All throw as the readers do.
    struct IdsOnly {};
    FastqStorage(IdsOnly, const std::string& ids_path);
    static void header_token(const char* s, size_t n, const char*& tok, size_t& tok_len);
    read_id_t resolve_token(const char* tok, size_t n) const { return resolve_id(tok, n); }
    read_id_t check_record(const char* const l1[4], const size_t n1[4], const char* const l2[4], const size_t n2[4], bool paired) const;

    // The stage's opt-in route (hc_ec_fastq_on_device): a storage whose files are read later.  EdgeCalculator's constructor either lets
    // the device read them into its store and hands over what hc_fastq_fetch returns (adopt: the ids, the offsets, the read vector and
    // m_ID_to_index — the bases and qualities stay on the device, and bases() / quals() fill themselves on first use by the host
    // reader's passes over the same files), or reads them here as the constructor above does (load_host).
    struct Deferred {};
    FastqStorage(Deferred, const ProgramSettings& ps);
    bool deferred() const { return m_deferred; }
    bool adopted() const { return m_lazy_bytes; }  // the device read the files (adopt)
    const ProgramSettings& deferred_settings() const { return m_ps; }
    void load_host();
    void adopt(const uint64_t* read_ids, const uint64_t* seq_off, const uint32_t* read_first_seq, uint32_t n_single, uint32_t n_paired);

private:
    void load(const ProgramSettings& ps);
    void index_reads();
    void fill_bytes() const;
    ProgramSettings m_ps;
    bool m_deferred = false, m_lazy_bytes = false;
    mutable std::once_flag m_fill_once;
    void read_new_ids(const std::string& path);
    void read_singles(const std::string& path, unsigned long max_reads);
    void read_pairs(const std::string& p1, const std::string& p2, unsigned long max_reads);
    void push_sequence(const char* s, size_t ns, const char* q, size_t nq, bool upper);
    // the same records from read-only mappings of the files, on several threads (regular files of some size); false: not
    // applicable, nothing was touched, the sequential readers take over
    bool read_mapped(const std::string& p1, const std::string* p2, unsigned long max_reads, unsigned threads);
    unsigned m_threads = 1;
    read_id_t resolve_id(const std::string& token) const;
    read_id_t resolve_id(const char* token, size_t n) const;

    std::map<std::string, std::string> m_new_readIDs;    // fastq id -> overlaps-file id (--IDs)
    bool m_have_new_ids = false;
    mutable ByteVec m_bases, m_quals;  // (mutable: the lazy fill)
    std::vector<uint64_t> m_seq_off{0};
    std::vector<uint32_t> m_first{0};
};

}  // namespace hc
