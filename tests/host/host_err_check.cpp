// Host check of csrc/host_err.h alone (tests/test_host_err_host.py builds it with -fsanitize=address,undefined and runs it):
// the message of the entry points that take no bcx_solver*.  No HIP header is on the include path, so the file has to stand alone.
#include <stdio.h>
#include <string.h>
#include <string>
#include <thread>
#include "../../bayesian-coresets_amd/csrc/host_err.h"

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_failed += 1; } } while (0)

static void test_grammar_and_code() {
  CHECK(strcmp(bcx_fail_text(), "") == 0);                          // before this thread's first failure
  CHECK(bcx_fail(-1, "bcx_gram", "bad arguments") == -1);
  CHECK(strcmp(bcx_fail_text(), "bcx_gram: bad arguments") == 0);
  for (int code : {-2, -5, -8, 0, 7}) CHECK(bcx_fail(code, "who", "what") == code);   // the code is passed through, whatever it is
  CHECK(strcmp(bcx_fail_text(), "who: what") == 0);
  // `what` built on the way in, with a colon of its own (the form of a HIP status: "<step>: <reason>")
  CHECK(bcx_fail(-2, "bcx_hmc_coreset", std::string("hipGetLastError()") + ": " + "invalid argument") == -2);
  CHECK(strcmp(bcx_fail_text(), "bcx_hmc_coreset: hipGetLastError(): invalid argument") == 0);
}

static void test_second_replaces_first() {
  bcx_fail(-1, "first", std::string(200, 'x'));                     // (long enough to live on the heap)
  bcx_fail(-5, "second", "short");
  CHECK(strcmp(bcx_fail_text(), "second: short") == 0);
  bcx_fail(-1, "third", std::string(500, 'y'));
  CHECK(bcx_fail_text() == "third: " + std::string(500, 'y'));
  // the old text as part of the new one: read before it is replaced
  bcx_fail(-1, "outer", std::string("inner failed: ") + bcx_fail_text());
  CHECK(bcx_fail_text() == "outer: inner failed: third: " + std::string(500, 'y'));
}

static void test_pointer_stays_valid() {
  bcx_fail(-1, "bcx_project", std::string(300, 'z'));
  const char* p = bcx_fail_text();
  const std::string copy(p);
  std::string noise;                                               // allocations in between must not disturb it
  for (int i = 0; i < 64; ++i) noise += std::string(100, (char)('a' + i % 26));
  CHECK(bcx_fail_text() == p);                                     // reading again: the same pointer, no copy handed out
  CHECK(copy == p && copy.size() == strlen("bcx_project: ") + 300);
  std::thread([] { bcx_fail(-1, "elsewhere", std::string(300, 'q')); }).join();   // another thread's failure is not this one's
  CHECK(bcx_fail_text() == p && copy == p);
  CHECK(noise.size() == 6400);
}

static void test_threads_read_their_own() {
  bcx_fail(-1, "main", "before the threads");
  std::string seen[2];
  const char* first[2] = {"", ""};
  bool fresh[2] = {false, false};
  auto body = [&](int t) {
    fresh[t] = strcmp(bcx_fail_text(), "") == 0;                    // a new thread starts with no message, whatever others hold
    for (int i = 0; i < 200; ++i) {
      const std::string what = "thread " + std::to_string(t) + " failure " + std::to_string(i);
      if (bcx_fail(-1 - t, "worker", what) != -1 - t || "worker: " + what != bcx_fail_text()) first[t] = "mismatch";
    }
    seen[t] = bcx_fail_text();
  };
  std::thread a(body, 0), b(body, 1);
  a.join(); b.join();
  CHECK(fresh[0] && fresh[1]);
  CHECK(strcmp(first[0], "") == 0 && strcmp(first[1], "") == 0);
  CHECK(seen[0] == "worker: thread 0 failure 199" && seen[1] == "worker: thread 1 failure 199");
  CHECK(strcmp(bcx_fail_text(), "main: before the threads") == 0);
}

static void test_empty_what() {
  CHECK(bcx_fail(-1, "bcx_gram", "") == -1);
  CHECK(strcmp(bcx_fail_text(), "bcx_gram: ") == 0);
  CHECK(bcx_fail(-1, "", "") == -1);
  CHECK(strcmp(bcx_fail_text(), ": ") == 0);
}

int main() {
  test_grammar_and_code();
  test_second_replaces_first();
  test_pointer_stays_valid();
  test_threads_read_their_own();
  test_empty_what();
  if (g_failed) { printf("HOST_ERR FAILED: %d checks\n", g_failed); return 1; }
  printf("HOST_ERR OK\n");
  return 0;
}
