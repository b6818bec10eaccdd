// drivers.h — what more than one of the driver files uses: host/drivers.cpp (makedb, query, count; the definitions),
// host/store_verbs.cpp (the verbs over a DB file's store) and host/cluster.cpp (cluster).
#pragma once

#include <string>
#include <thread>
#include <vector>

#include "../engine.h"
#include "fastx.h"

namespace smafa {

struct DbGuard {
    smafa_db *db = nullptr;
    ~DbGuard() { smafa_db_destroy(db); }
};

struct FreeGuard {
    void *p = nullptr;
    ~FreeGuard() { smafa_free(p); }
};

#pragma GCC visibility push(hidden)  // internal to the library: nothing below is exported

int write_all(int fd, const char *p, size_t n);  // all n bytes to fd, or SMAFA_ERR_IO
void append_u32(std::string &s, uint32_t v);     // v in decimal
// does the DB file start like a packed store file (host/packed.cpp)?  Unreadable files are left to the reader that follows.
bool db_file_is_packed(const char *db_path);

// Device bring-up (warm_device) on helper threads, one per distinct device, while the caller reads and decodes its input; joined
// before the first device call, and by the destructor on any other way out.
class WarmDevices {
    std::vector<std::thread> t;

  public:
    WarmDevices(const int *devices, int ndev) {
        for (int g = 0; g < ndev; g++) {
            bool seen = false;
            for (int h = 0; h < g; h++) seen = seen || devices[h] == devices[g];
            if (!seen) t.emplace_back(warm_device, devices[g]);
        }
    }
    explicit WarmDevices(int device) : WarmDevices(&device, 1) {}
    void join() {
        for (auto &th : t)
            if (th.joinable()) th.join();
    }
    ~WarmDevices() { join(); }
};

// "Cannot compute distances between seq of length {len} and windows of lengths {store_len}": get_distances, src/lib.rs:72-79
std::string length_panic_text(size_t len, size_t store_len);
// What the record that stopped a bulk load (recs.err_kind) fails the run with, once the rows of the records before it are out:
// -> SMAFA_OK, or SMAFA_ERR_PANIC with the reference's text in `msg`.  noun: "query" / "input", for the parse failure;
// store_len: the length the records are held against.  An empty first record is reported as it is for cluster, where it would
// become a centroid (push_encoding, src/lib.rs:103-108); query, where it fails the length check, says so itself.
int pending_panic(const BulkRecords &recs, const char *noun, size_t store_len, std::string &msg);

#pragma GCC visibility pop
}  // namespace smafa
