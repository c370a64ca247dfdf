// cli_main.cpp -- `ecoz2 vq {learn,quantize,show}` front-end over libecoz2vq.so.
// Mirrors the reference's clap option structs for this path
// (/root/reference/src/vq/mod.rs:38-96 VqLearnOpts / VqQuantizeOpts, :120-133 VqShowOpts)
// and its mains (:151-216): same flag names, defaults, file-list resolution and messages.
// Like the reference (src/vq/mod.rs:146-148) errors are printed and the exit code stays 0
// unless the arguments themselves are unusable.
#include "../../include/ecoz2_classify.h"
#include "../../include/ecoz2_vq.h"
#include "vq_io.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <climits>
#include <set>
#include <cmath>
#include <string>
#include <vector>

static void callback(void*, int M, double avg, double sigma, double inertia)
{
    // Ecoz2ObserverRef::step, src/ecoz2_lib/mod.rs:61-69
    printf("   Ecoz2ObserverRef.step: M=%d avg_distortion=%g sigma=%g inertia=%g\n", M, avg, sigma, inertia);
}

static int usage()
{
    fprintf(stderr,
            "usage:\n"
            "  ecoz2 vq learn [-B <codebook>] [-P <P>] [-e <eps>] [--class-name <class>] [--exp-key <k>]\n"
            "                 --predictors <files|dirs|tt.csv>...\n"
            "  ecoz2 vq learn --all-classes -P <P> [-e <eps>] --predictors <files|dirs|tt.csv>...   (one codebook per class,\n"
            "                 trained together)\n"
            "  ecoz2 vq quantize --codebook <cbook> --predictors <files|dirs|tt.csv>...\n"
            "                 [--predictors-dir-template <t>] [--tt <TRAIN|TEST>] [--class-name <class>] [-s]\n"
            "  ecoz2 vq quantize --codebooks <files|dirs>... --predictors <files|dirs|tt.csv>...   (every codebook in one pass,\n"
            "                 [--tt <TRAIN|TEST>] [--class-name <class>] [-s]                      ascending M)\n"
            "  ecoz2 vq classify [-r] --codebooks <files|dirs>... --tt <TRAIN|TEST> --predictors <files|dirs|tt.csv>...\n"
            "  ecoz2 vq show [-f <from>] [-t <to>] <codebook>\n"
            "  ecoz2 seq show [-c] [-L] [--full] [--pickle out.pkl -M <M> --tt <TRAIN|TEST> [--class-name c]] <file.seq|tt.csv>...\n"
            "  ecoz2 seq show [-P] [-Q] --hmm <model> [-c] [-L] [--full] <file.seq>...\n"
            "  ecoz2 prd show [-k] [--predictors] [--cepstrum <Q>] [-f|--from a] [-t|--to b] [--zrs] [--pickle <out.pkl>]\n"
            "                 <file.prd|predictor.cbor>\n"
            "  ecoz2 {nb|mm} learn -M <M> [--class-name <class>] <file.seq|dirs|tt.csv>...\n"
            "  ecoz2 {nb|mm} classify -M <M> [-r] --tt <TRAIN|TEST> --models <files|dirs>... --sequences <files|dirs|tt.csv>...\n"
            "  ecoz2 {nb|mm} show --model <file>\n"
            "  ecoz2 hmm learn [-N 5] -M <M> [-t 3] [-I -1] [-e 1e-05] [-a 0.3] [-s <seed>] [--ser] [--class-name c]\n"
            "                  --sequences <file.seq|dirs|tt.csv>...\n"
            "  ecoz2 hmm learn --all-classes [-N 5] -M <M> [-t 3] [-I -1] [-e 1e-05] [-a 0.3] [-s <seed>]\n"
            "                  --sequences <file.seq|dirs|tt.csv>...   (one model per class, trained together)\n"
            "  ecoz2 hmm learn --grid -N <n1,n2,...> -M <m1,m2,...> [-t 3] [-I -1] [-e 1e-05] [-a 0.3] [-s <seed>]\n"
            "                  --sequences <file.seq|dirs|tt.csv>...   (one model per N, M and class, trained together)\n"
            "  ecoz2 hmm learn --embedded -m|--models <files|dirs>... --labels <files>... [--filler <class>] [--switch-penalty <x <= 0>]\n"
            "                  [-e 1e-05] [-a 0.3] [-I -1] -o <dir> [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n"
            "                  [--body <auto|resident|looped>]\n"
            "                  (--signals <.wav files>... | --predictors <.prd files>... | --sequences <.seq files>...)\n"
            "                  (the given models re-estimated from whole recordings and the order of their units, no boundaries:\n"
            "                  label file i is recording i's transcript, as `hmm align` reads it; the models go to <dir>/<class>.hmm)\n"
            "  ecoz2 hmm learn --loop -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15] --switch-penalty <x <= 0 | -inf>\n"
            "                  [--class-transitions <file.csv>] [--train-transitions [--alpha 1]] [--freeze <class>]... [-e 1e-05] [-a 0.3]\n"
            "                  [-I -1] -o <dir> --sequences <.seq>... | --predictors <.prd>... | --signals <.wav>...\n"
            "                  (the given models re-estimated from whole unlabelled recordings under the class loop `hmm segment\n"
            "                  --class-transitions` decodes, with --train-transitions the matrix too; --freeze: that class's model stays;\n"
            "                  the models go to <dir>/<class>.hmm, the matrix to <dir>/transitions.csv, the history to <dir>/loop.csv)\n"
            "  ecoz2 hmm classify [-r] [-c|--c12n <out.csv>] -m|--models <files|dirs>... --tt <TRAIN|TEST> -M <M> [--class-name c]\n"
            "                  (-s|--sequences <files|dirs|tt.csv>... | --predictors <files|dirs|tt.csv>... --codebooks <files|dirs>...\n"
            "                   [--predictors-dir-template <t>])\n"
            "  ecoz2 hmm classify --grid [-r] [-c|--c12n <dir>] [--summary <file.csv>] -m|--models <files|dirs>... --tt <TRAIN|TEST>\n"
            "                  [-M <m1,m2,...>] -s|--sequences <files|dirs|tt.csv>...   (every (N, M) of the models, scored together;\n"
            "                  a tt.csv needs -M)\n"
            "  ecoz2 hmm scan -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15] --window <frames>\n"
            "                  [--hop <frames>] [--min-margin <x>] [-c <csv dir|file.csv>]\n"
            "                  (--signals <.wav files|dirs>... | --predictors <.prd files|dirs>... | --sequences <.seq files|dirs>...)\n"
            "                  (where in each recording every class occurs: the models over sliding windows; --hop defaults to --window)\n"
            "  ecoz2 hmm segment -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n"
            "                  --switch-penalty <x <= 0 | -inf> [-c <csv dir|file.csv>]\n"
            "                  [--posteriors [--frame-posteriors <dir>]]\n"
            "                  [--body <auto|resident|looped>]\n"
            "                  [--class-transitions <file.csv>]\n"
            "                  [--grammar-posteriors [--frame-posteriors <dir>]]\n"
            "                  [--continuous <name>]\n"
            "                  [--grammar-body <auto|resident|looped>]\n"
            "                  [--grammar-posteriors-body <auto|resident|looped>]\n"
            "                  (--signals <.wav files|dirs>... | --predictors <.prd files|dirs>... | --sequences <.seq files|dirs>...)\n"
            "                  (each recording decoded once under all models: segment boundaries to the frame, a class per segment;\n"
            "                  --posteriors adds each segment's mean and least class posterior, and the per-frame table)\n"
            "                  (--body, with --posteriors: the kernel body of the posteriors -- resident takes at most 16 wave-slots\n"
            "                  of classes, looped any number, auto the looped one above 16; the figures are the same bit for bit)\n"
            "                  (--class-transitions adds the file's price of every class-to-class succession to the penalty)\n"
            "                  (--grammar-posteriors, with --class-transitions: the posteriors under those prices, reported as\n"
            "                  --posteriors reports them)\n"
            "                  (--continuous <name>: the inputs are consecutive pieces of one recording, decoded as one stream)\n"
            "                  (--grammar-body, with --class-transitions: the kernel body of the decoder under the prices -- resident\n"
            "                  takes at most 16 wave-slots of classes, looped any number, auto the looped one above 16; the same path\n"
            "                  bit for bit; not with --grammar-posteriors)\n"
            "                  (--grammar-posteriors-body, with --grammar-posteriors: the kernel body of the posteriors under the prices,\n"
            "                  which the decode of the same recording follows -- resident takes at most 16 wave-slots of classes, looped\n"
            "                  any number, auto the looped one above 16; the figures are the same bit for bit)\n"
            "  ecoz2 hmm segment -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n"
            "                  --switch-penalty <x <= 0 | -inf> --class-transitions <file.csv> --grammar-continuous <name>\n"
            "                  [-c <csv dir|file.csv>]\n"
            "                  [--grammar-body <auto|resident|looped>]\n"
            "                  (--signals <.wav files|dirs>... | --predictors <.prd files|dirs>... | --sequences <.seq files|dirs>...)\n"
            "                  (--grammar-continuous <name>: the inputs are consecutive pieces of one recording, decoded as one stream\n"
            "                  under the prices of --class-transitions)\n"
            "  ecoz2 hmm segment -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n"
            "                  --switch-penalty <x <= 0 | -inf> --continuous-posteriors <name> [--block 4096] [--lookahead 4096]\n"
            "                  [--frame-posteriors <dir>] [--body <auto|resident|looped>] [-c <csv dir|file.csv>]\n"
            "                  (--signals <.wav files|dirs>... | --predictors <.prd files|dirs>... | --sequences <.seq files|dirs>...)\n"
            "                  (--continuous-posteriors <name>: the inputs are consecutive pieces of one recording, decoded as one stream\n"
            "                  and reported as --posteriors reports a recording; the posteriors of a block of --block frames are\n"
            "                  computed once --lookahead frames behind it are known, and are conditioned on the recording up to there:\n"
            "                  a look-ahead of at least the recording's length gives the figures of --posteriors bit for bit)\n"
            "  ecoz2 hmm transitions -m|--models <files|dirs>... [--alpha 1] -o <file.csv> <segment .csv | selection table>...\n"
            "                  (the class-to-class prices for --class-transitions, from the successions of labelled segments)\n"
            "  ecoz2 hmm transitions --em -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15] --switch-penalty <x>\n"
            "                  [--init <file.csv>] [--alpha 1] [-a val_auto] [-I max_iterations] -o <file.csv>\n"
            "                  --sequences <.seq>... | --predictors <.prd>... | --signals <.wav>...\n"
            "                  [--body <auto|resident|looped>]\n"
            "                  (the same prices by Baum-Welch from unlabelled recordings under the models; <file.csv>.em.csv: the iterations)\n"
            "                  (--body: the kernel body of the E-step -- resident takes at most 16 wave-slots of classes, looped any\n"
            "                  number, auto the looped one above 16; the same matrix bit for bit)\n"
            "  ecoz2 hmm align -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n"
            "                  [--switch-penalty <x <= 0>] [--filler <class>] [-c <csv dir|file.csv>] --labels <files>...\n"
            "                  [--posteriors [--frame-posteriors <dir>]]\n"
            "                  [--body <auto|resident|looped>]\n"
            "                  (--signals <.wav files>... | --predictors <.prd files>... | --sequences <.seq files>...)\n"
            "                  (each recording aligned to the units its label file names, in their order: a segment .csv or a\n"
            "                  selection table; --filler: that class's model may stand before, between and after the units;\n"
            "                  --posteriors adds how sure each unit is: the path's mean and least posterior over its frames, the\n"
            "                  probability that the unit is there, the mean and spread of its first frame; and the per-frame table;\n"
            "                  --body, with --posteriors: the kernel body of the posteriors -- resident takes a transcript of at most\n"
            "                  16 wave-slots, looped any number, auto the looped one above 16; the same posteriors bit for bit)\n"
            "  ecoz2 hmm show --hmm <file> [-f|--format \"%%Lg \"]\n"
            "  ecoz2 lpc [-P 36] [-W 45] [-O 15] [-m 0] [-s 0] [-X 5] [--verbose] --signals <files|dirs|tt.csv>...\n"
            "            [--signals-dir-template data/signals] [--tt <TRAIN|TEST>] [--class <class>]\n"
            "  ecoz2 cversion\n");
    return 2;
}

static bool is_flag(const char* a) { return a[0] == '-' && a[1] != 0 && !(a[1] >= '0' && a[1] <= '9'); }

static std::vector<const char*> cptrs(const std::vector<std::string>& v)
{
    std::vector<const char*> p;
    for (const auto& s : v) p.push_back(s.c_str());
    return p;
}

static int vq_learn(int argc, char** argv)
{
    std::string base, cls, exp_key;
    int P = -1;
    double eps = 0.05;
    std::vector<std::string> predictors;
    bool all_classes = false;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        if (a == "--all-classes") all_classes = true;
        else if (a == "-B" || a == "--base-codebook") base = val("-B");
        else if (a == "-P" || a == "--prediction-order") P = atoi(val("-P"));
        else if (a == "-e" || a == "--epsilon") eps = atof(val("-e"));
        else if (a == "--class-name") cls = val("--class-name");
        else if (a == "--exp-key") exp_key = val("--exp-key");
        else if (a == "--predictors") { while (i + 1 < argc && !is_flag(argv[i + 1])) predictors.push_back(argv[++i]); }
        else if (!is_flag(argv[i])) predictors.push_back(a);
        else return usage();
    }
    if (all_classes) {  // every class of the TRAIN rows / given files at once
        if (!cls.empty() || !base.empty()) {
            fprintf(stderr, "--all-classes excludes --class-name and -B\n");
            return usage();
        }
        if (P < 0) return usage();
        std::vector<std::string> files;
        const bool tt_list = predictors.size() == 1 && predictors[0].size() > 4 &&
                             predictors[0].compare(predictors[0].size() - 4, 4, ".csv") == 0;
        int rc = tt_list ? e2vq_io::files_from_csv(predictors[0], "TRAIN", "", "predictors", ".prd", nullptr, files)
                         : e2vq_io::resolve_filenames(predictors, ".prd", files);
        if (!rc && files.empty()) { printf("No predictors given\n"); return 0; }
        if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
        std::set<std::string> classes;
        for (const std::string& f : files) {
            char c[96];
            int p;
            int64_t T;
            if (e2vq_prd_info(f.c_str(), c, &p, &T)) { printf("%s\n", e2vq_last_error()); return 0; }
            classes.insert(c);
        }
        printf("predictor files: %zu\n", files.size());
        printf("classes: %zu\n", classes.size());
        auto ptrs = cptrs(files);
        if (e2vq_vq_learn_classes(P, eps, ptrs.data(), (int)ptrs.size(), nullptr, callback)) printf("%s\n", e2vq_last_error());
        return 0;
    }
    if (!base.empty() && P >= 0) {  // src/vq/mod.rs:161-163
        printf("Only one of base codebook or prediction order expected\n");
        return 0;
    }
    if (base.empty() && P < 0) return usage();
    const std::string codebook_class = cls.empty() ? "_" : cls;
    std::vector<std::string> files;
    const bool tt_list = predictors.size() == 1 && predictors[0].size() > 4 &&
                         predictors[0].compare(predictors[0].size() - 4, 4, ".csv") == 0;
    int rc = tt_list ? e2vq_io::files_from_csv(predictors[0], "TRAIN", cls, "predictors", ".prd", nullptr, files)
                     : e2vq_io::resolve_filenames(predictors, ".prd", files);
    if (!rc && files.empty()) { printf("No predictors given\n"); return 0; }
    if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
    printf("vq_learn: base_codebook_opt=%s prediction_order=%d, epsilon=%g codebook_class_name=%s predictor_filenames: %zu\n",
           base.empty() ? "None" : base.c_str(), P, eps, codebook_class.c_str(), files.size());
    auto ptrs = cptrs(files);
    if (!base.empty())
        ecoz2_vq_learn_using_base_codebook(base.c_str(), eps, ptrs.data(), (int)ptrs.size(), nullptr, callback);
    else
        ecoz2_vq_learn(P, eps, codebook_class.c_str(), ptrs.data(), (int)ptrs.size(), nullptr, callback);
    return 0;
}

static int vq_quantize(int argc, char** argv)
{
    std::string codebook, tmpl = "data/predictors", tt, cls;
    bool show = false;
    std::vector<std::string> predictors, codebooks;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        if (a == "--codebook") codebook = val("--codebook");
        else if (a == "--codebooks") { while (i + 1 < argc && !is_flag(argv[i + 1])) codebooks.push_back(argv[++i]); }
        else if (a == "--predictors-dir-template") tmpl = val("--predictors-dir-template");
        else if (a == "--tt") tt = val("--tt");
        else if (a == "--class-name") cls = val("--class-name");
        else if (a == "-s" || a == "--show-filenames") show = true;
        else if (a == "--predictors") { while (i + 1 < argc && !is_flag(argv[i + 1])) predictors.push_back(argv[++i]); }
        else if (!is_flag(argv[i])) predictors.push_back(a);
        else return usage();
    }
    if (codebook.empty() == codebooks.empty() || predictors.empty()) return usage();  // (one of --codebook / --codebooks)
    std::vector<std::string> files, cbs;
    if (!codebooks.empty()) {
        e2vq_io::resolve_filenames(codebooks, ".cbook", cbs);
        if (cbs.empty()) { printf("No codebooks given\n"); return 0; }
    }
    const bool tt_list = predictors.size() == 1 && predictors[0].size() > 4 &&
                         predictors[0].compare(predictors[0].size() - 4, 4, ".csv") == 0;
    int rc = tt_list ? e2vq_io::files_from_csv(predictors[0], tt, cls, "", ".prd", &tmpl, files)
                     : e2vq_io::resolve_filenames(predictors, ".prd", files);
    if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
    printf("number of predictor files: %zu\n", files.size());  // src/vq/mod.rs:211
    auto ptrs = cptrs(files);
    if (!cbs.empty()) {
        for (const std::string& c : cbs) printf("nom_raas = %s\n", c.c_str());
        auto pc = cptrs(cbs);
        e2vq_vq_quantize_codebooks(pc.data(), (int)pc.size(), ptrs.data(), (int)ptrs.size(), show ? 1 : 0);
        return 0;
    }
    printf("nom_raas = %s\n", codebook.c_str());               // src/ecoz2_lib/mod.rs:326
    ecoz2_vq_quantize(codebook.c_str(), ptrs.data(), (int)ptrs.size(), show ? 1 : 0);
    return 0;
}

static int vq_classify(int argc, char** argv)
{
    bool ranked = false;
    std::string tt;
    std::vector<std::string> codebooks, predictors;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-r" || a == "--show-ranked") ranked = true;
        else if (a == "--tt" && i + 1 < argc) tt = argv[++i];
        else if (a == "--codebooks") { while (i + 1 < argc && !is_flag(argv[i + 1])) codebooks.push_back(argv[++i]); }
        else if (a == "--predictors") { while (i + 1 < argc && !is_flag(argv[i + 1])) predictors.push_back(argv[++i]); }
        else return usage();
    }
    if (codebooks.empty() || predictors.empty() || tt.empty()) return usage();
    std::vector<std::string> cbs, prds;
    e2vq_io::resolve_filenames(codebooks, ".cbook", cbs);
    if (cbs.empty()) { printf("No codebooks given\n"); return 0; }
    const bool tt_list = predictors.size() == 1 && predictors[0].size() > 4 &&
                         predictors[0].compare(predictors[0].size() - 4, 4, ".csv") == 0;
    int rc = tt_list ? e2vq_io::files_from_csv(predictors[0], tt, "", "predictors", ".prd", nullptr, prds)
                     : e2vq_io::resolve_filenames(predictors, ".prd", prds);
    if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
    if (prds.empty()) { printf("No predictors given\n"); return 0; }
    printf("number of codebooks: %zu  number of predictors: %zu\n", cbs.size(), prds.size());  // src/vq/mod.rs:236-241
    printf("show_ranked = %s\n", ranked ? "true" : "false");
    auto pc = cptrs(cbs), pp = cptrs(prds);
    ecoz2_vq_classify(pc.data(), (int)pc.size(), pp.data(), (int)pp.size(), ranked ? 1 : 0);
    return 0;
}

static int vq_show(int argc, char** argv)
{
    int from = -1, to = -1;
    std::string codebook;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        if ((a == "-f" || a == "--from") && i + 1 < argc) from = atoi(argv[++i]);
        else if ((a == "-t" || a == "--to") && i + 1 < argc) to = atoi(argv[++i]);
        else if (a == "--codebook" && i + 1 < argc) codebook = argv[++i];
        else codebook = a;
    }
    if (codebook.empty()) return usage();
    printf("codebook_filename = %s\n", codebook.c_str());  // src/ecoz2_lib/mod.rs:361
    ecoz2_vq_show(codebook.c_str(), from, to);
    return 0;
}

// `ecoz2 seq show [-c] [-L] [--full] <files...>`: Sequence::show, /root/reference/src/sequence/mod.rs:17-47
// (reads the C-format .seq exactly as Sequence::load does, :49-75)
static bool load_seq(const std::string& f, std::string& cls, unsigned& M, std::vector<unsigned>& sym)
{
    FILE* fp = fopen(f.c_str(), "rb");
    unsigned char hdr[120];
    if (!fp || fread(hdr, 1, sizeof hdr, fp) != sizeof hdr || strncmp((const char*)hdr, "<sequence>", 10) != 0) {
        if (fp) fclose(fp);
        return false;
    }
    char c[97] = {0};
    memcpy(c, hdr + 16, 96);
    cls = c;
    const unsigned len = hdr[112] | (hdr[113] << 8) | (hdr[114] << 16) | ((unsigned)hdr[115] << 24);
    M = hdr[116] | (hdr[117] << 8) | (hdr[118] << 16) | ((unsigned)hdr[119] << 24);
    sym.assign(len, 0);
    for (unsigned t = 0; t < len; ++t) {
        unsigned char b[2];
        if (fread(b, 1, 2, fp) != 2) break;
        sym[t] = b[0] | (b[1] << 8);
    }
    fclose(fp);
    return true;
}

// pickle (protocol 2) of a list of lists of ints or floats: what `utl::to_pickle(&list, ..)` exports
// (the reference's src/seq/mod.rs:88-112, src/prd/mod.rs:174-188, src/utl/mod.rs:277-283); loads with Python's pickle.load
static void pickle_item(FILE* fp, unsigned v)
{
    if (v < 256) { fputc('K', fp); fputc((int)v, fp); }                                   // BININT1
    else if (v < 65536) { fputc('M', fp); fputc(v & 255, fp); fputc(v >> 8, fp); }        // BININT2
    else { fputc('J', fp); for (int k = 0; k < 4; ++k) fputc((v >> (8 * k)) & 255, fp); } // BININT
}

static void pickle_item(FILE* fp, double v)
{
    uint64_t u;
    memcpy(&u, &v, 8);
    fputc('G', fp);  // BINFLOAT: big-endian IEEE double
    for (int k = 7; k >= 0; --k) fputc((int)((u >> (8 * k)) & 255), fp);
}

template <typename V>
static bool write_pickle(const std::string& path, const std::vector<std::vector<V>>& lists)
{
    FILE* fp = fopen(path.c_str(), "wb");
    if (!fp) return false;
    fputc(0x80, fp); fputc(2, fp);  // PROTO 2
    fputc(']', fp);                 // EMPTY_LIST
    fputc('(', fp);                 // MARK
    for (const auto& s : lists) {
        fputc(']', fp);
        fputc('(', fp);
        for (const V& v : s) pickle_item(fp, v);
        fputc('e', fp);             // APPENDS
    }
    fputc('e', fp);
    fputc('.', fp);                 // STOP
    return fclose(fp) == 0;
}

// With -P (forward ln P) or -Q (Viterbi path and its ln P*) under --hmm <model>: e2vq_seq_show_files, on the GPU
static int seq_show(int argc, char** argv)
{
    bool no_sequence = false, only_length = false, full = false, with_prob = false, gen_q_opt = false;
    std::string pickle, cls_filter, tt, hmm;
    int codebook_size = -1;
    std::vector<std::string> files;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-c") no_sequence = true;
        else if (a == "-L") only_length = true;
        else if (a == "--full") full = true;
        else if (a == "-P") with_prob = true;
        else if (a == "-Q") gen_q_opt = true;
        else if (a == "--hmm" && i + 1 < argc) hmm = argv[++i];
        else if (a == "--pickle" && i + 1 < argc) pickle = argv[++i];
        else if (a == "--class-name" && i + 1 < argc) cls_filter = argv[++i];
        else if (a == "--tt" && i + 1 < argc) tt = argv[++i];
        else if ((a == "-M" || a == "--codebook-size") && i + 1 < argc) codebook_size = atoi(argv[++i]);
        else if (!is_flag(argv[i])) files.push_back(a);
        else return usage();
    }
    if (files.empty()) return usage();
    if (with_prob || gen_q_opt) {
        if (!pickle.empty()) {
            fprintf(stderr, "-P / -Q cannot be combined with --pickle\n");
            return 2;
        }
        if (hmm.empty()) {
            fprintf(stderr, "-P / -Q need a model: --hmm <file.hmm>\n");
            return 2;
        }
        auto ps = cptrs(files);
        if (e2vq_seq_show_files(with_prob, gen_q_opt, no_sequence, hmm.c_str(), ps.data(), (int)ps.size(), full, only_length)) {
            printf("%s\n", e2vq_last_error());
            return 1;
        }
        return 0;
    }
    if (!pickle.empty()) {  // src/seq/mod.rs:88-118
        if (codebook_size < 0 || tt.empty()) {
            printf("--codebook-size and --tt required when --pickle given\n");
            return 0;
        }
        std::vector<std::string> seq_files;
        const bool tt_list = files.size() == 1 && files[0].size() > 4 && files[0].compare(files[0].size() - 4, 4, ".csv") == 0;
        const std::string subdir = "sequences/M" + std::to_string(codebook_size);
        int rc = tt_list ? e2vq_io::files_from_csv(files[0], tt, cls_filter, subdir, ".seq", nullptr, seq_files)
                         : e2vq_io::resolve_filenames(files, ".seq", seq_files);
        if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
        std::vector<std::vector<unsigned>> seqs;
        for (const auto& f : seq_files) {
            std::string cls; unsigned M; std::vector<unsigned> sym;
            if (!load_seq(f, cls, M, sym)) { printf("%s: Not a sequence\n", f.c_str()); return 0; }
            seqs.push_back(sym);
        }
        if (!write_pickle(pickle, seqs)) { printf("%s: cannot write\n", pickle.c_str()); return 0; }
        printf("%zu sequence(s) saved to \"%s\"\n", seqs.size(), pickle.c_str());
        return 0;
    }
    for (const auto& f : files) {
        std::string cls_s;
        unsigned M = 0;
        std::vector<unsigned> sym;
        if (!load_seq(f, cls_s, M, sym)) {
            printf("%s: Not a sequence\n", f.c_str());
            continue;
        }
        const char* cls = cls_s.c_str();
        const unsigned len = (unsigned)sym.size();
        if (no_sequence) continue;
        if (only_length) { printf("%u\n", len); continue; }
        printf("<%s(M=%u,L=%u): ", cls, M, len);
        if (full || len <= 30) {
            for (unsigned t = 0; t < len; ++t) printf("%s%u", t ? ", " : "", sym[t]);
        } else {
            for (unsigned t = 0; t < 10; ++t) printf("%s%u", t ? ", " : "", sym[t]);
            printf(", ..., ");
            for (unsigned t = len - 10; t < len; ++t) printf("%s%u", t > len - 10 ? ", " : "", sym[t]);
        }
        printf(">\n");
    }
    return 0;
}

// `ecoz2 prd show [--predictors] [-k|--reflections] [--cepstrum Q] [-f|--from a] [-t|--to b] [--zrs] [--pickle FILE]
// <file>` (options: src/prd/mod.rs:30-62; from defaults to 1, to = 0 means the last column).  Without the new options:
// ecoz2_prd_show_file, the symbol the reference binds (src/ecoz2_lib/mod.rs:89-94, src/prd/mod.rs:99), unchanged.
// With any of --predictors, --cepstrum, --pickle or --zrs: prd_show_rs / Predictor::show (src/prd/mod.rs:105-225) on
// the same frames, the features computed by e2vq_lpc_features; the input may also be a CBOR predictor document.

// Rust's `{:.4e}` (|v| < 0.00001) or `{:.5}` of an f64: exponent without '+' or padding, NaN, inf, -inf
static void put_rust(double v)
{
    if (std::isnan(v)) { fputs("NaN", stdout); return; }
    if (std::isinf(v)) { fputs(v < 0 ? "-inf" : "inf", stdout); return; }
    char buf[64];
    if (fabs(v) < 0.00001) {
        snprintf(buf, sizeof buf, "%.4e", v);
        char* e = strchr(buf, 'e');
        snprintf(e, sizeof buf - (size_t)(e - buf), "e%d", atoi(e + 1));
    } else {
        snprintf(buf, sizeof buf, "%.5f", v);
    }
    fputs(buf, stdout);
}

static int device_of_env()
{
    const char* v = getenv("ECOZ2_VQ_DEVICE");
    return v && *v ? atoi(v) : 0;
}

static bool parse_count(const char* v, long* out)
{
    char* end = nullptr;
    const long x = strtol(v, &end, 10);
    if (!*v || *end || x < 0 || x > 1000000000L) return false;
    *out = x;
    return true;
}

static int prd_show_rs(const std::string& file, bool predictors, bool refl, long cepstrum, long from, long to,
                       const std::string& pickle)
{
    std::string cls;
    int P = 0;
    std::vector<double> r;
    if (e2vq_io::predictor_load(file.c_str(), cls, P, r)) { printf("%s\n", e2vq_last_error()); return 0; }
    const int NC = P + 1;
    const int64_t T = (int64_t)(r.size() / (size_t)NC);
    printf("# %s\n", file.c_str());
    if (cepstrum >= 0 && cepstrum <= P) {
        fflush(stdout);
        fprintf(stderr, "cepstrum value=%ld must be > prediction order=%d", cepstrum, P);
        return 0;
    }
    const int Q = cepstrum > 0 ? (int)std::min<long>(cepstrum, INT32_MAX) : 0;
    long to_;
    const char* name;
    int width;  // values per vector
    std::vector<double> feat;
    std::vector<int32_t> status;
    std::vector<double> pe;
    int rc = 0;
    if (Q > 0) {
        to_ = to == 0 || to >= Q ? Q - 1 : to;
        name = "c";
        width = Q;
        if (Q > E2VQ_LPC_FEATURES_MAX_Q) {
            fprintf(stderr, "cepstrum value=%d exceeds the limit of %d\n", Q, E2VQ_LPC_FEATURES_MAX_Q);
            return 1;
        }
        feat.resize((size_t)T * Q);
        status.resize((size_t)T);
        pe.resize((size_t)T);
        rc = e2vq_lpc_features(device_of_env(), P, Q, r.data(), T, status.data(), pe.data(), nullptr,
                               nullptr, feat.data(), 0);
    } else {
        to_ = to == 0 || to > P ? P : to;
        name = predictors ? "a" : refl ? "k" : "r";
        width = NC;
        if (predictors || refl) {
            feat.resize((size_t)T * NC);
            rc = e2vq_lpc_features(device_of_env(), P, 0, r.data(), T, nullptr, nullptr,
                                   refl && !predictors ? feat.data() : nullptr, predictors ? feat.data() : nullptr,
                                   nullptr, 0);
        } else {
            feat.swap(r);
        }
    }
    if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
    for (int64_t t = 0; t < (int64_t)status.size(); ++t)  // get_cepstrum's warnings (src/prd/mod.rs:252-257)
        if (status[t] != 0) fprintf(stderr, "WARNING: lpca_r: res_lpca = %d, err_pred = %.17g\n", status[t], pe[t]);
    if (from > to_ + 1) {  // Rust: a slice-index panic
        fflush(stdout);
        fprintf(stderr, "range %ld..=%ld out of bounds for vectors of length %d\n", from, to_, width);
        return 1;
    }
    if (!pickle.empty()) {
        std::vector<std::vector<double>> list((size_t)T);
        for (int64_t t = 0; t < T; ++t)
            list[(size_t)t].assign(feat.begin() + t * width + from, feat.begin() + t * width + to_ + 1);
        if (!write_pickle(pickle, list)) { printf("%s: cannot write\n", pickle.c_str()); return 0; }
        printf("%lld vectors(s) saved to \"%s\"\n", (long long)T, pickle.c_str());
        return 0;
    }
    printf("# class_name='%s', T=%lld P=%d\n", cls.c_str(), (long long)T, P);
    for (long i = from; i <= to_; ++i) printf("%s%s%ld", i == from ? "" : ",", name, i);
    printf("\n");
    for (int64_t t = 0; t < T; ++t) {
        const double* v = feat.data() + t * width;
        for (long i = from; i <= to_; ++i) {
            if (i > from) fputs(", ", stdout);
            put_rust(v[i]);
        }
        printf("\n");
    }
    return 0;
}

static int prd_show(int argc, char** argv)
{
    long from = 1, to = 0, cepstrum = -1;
    int refl = 0;
    bool predictors = false, zrs = false;
    std::string file, pickle;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        if ((a == "--from" || a == "-f") && i + 1 < argc) { if (!parse_count(argv[++i], &from)) return usage(); }
        else if ((a == "--to" || a == "-t") && i + 1 < argc) { if (!parse_count(argv[++i], &to)) return usage(); }
        else if (a == "-k" || a == "--reflections") refl = 1;
        else if (a == "--predictors") predictors = true;
        else if (a == "--cepstrum" && i + 1 < argc) { if (!parse_count(argv[++i], &cepstrum)) return usage(); }
        else if (a == "--pickle" && i + 1 < argc) pickle = argv[++i];
        else if (a == "--zrs") zrs = true;
        else if (!is_flag(argv[i])) file = a;
        else return usage();
    }
    if (file.empty()) return usage();
    if (predictors || cepstrum >= 0 || !pickle.empty() || zrs) return prd_show_rs(file, predictors, refl, cepstrum, from, to, pickle);
    ecoz2_prd_show_file(file.c_str(), refl, (int)from, (int)to);
    return 0;
}

// `ecoz2 nb ...` / `ecoz2 mm ...`: option structs and mains of /root/reference/src/nb/mod.rs:32-161 and
// src/mm/mod.rs:32-161 (identical shapes; the models differ)
static bool is_csv_list(const std::vector<std::string>& v)
{
    return v.size() == 1 && v[0].size() > 4 && v[0].compare(v[0].size() - 4, 4, ".csv") == 0;
}

static int seq_model_cmd(bool nb, int argc, char** argv)
{
    if (argc < 1) return usage();
    const std::string cmd = argv[0];
    const char* ext = nb ? ".nb" : ".mm";
    int M = -1;
    bool ranked = false;
    std::string cls, tt, model;
    std::vector<std::string> models, sequences;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if ((a == "-M" || a == "--codebook-size") && i + 1 < argc) M = atoi(argv[++i]);
        else if ((a == "--class-name") && i + 1 < argc) cls = argv[++i];
        else if (a == "-r" || a == "--show-ranked") ranked = true;
        else if (a == "--tt" && i + 1 < argc) tt = argv[++i];
        else if ((a == "-m" || a == "--model") && i + 1 < argc) model = argv[++i];
        else if (a == "--models") { while (i + 1 < argc && !is_flag(argv[i + 1])) models.push_back(argv[++i]); }
        else if (a == "--sequences") { while (i + 1 < argc && !is_flag(argv[i + 1])) sequences.push_back(argv[++i]); }
        else if (!is_flag(argv[i])) sequences.push_back(a);
        else return usage();
    }
    if (cmd == "show") {
        if (model.empty()) return usage();
        if (nb ? ecoz2_nb_show(model.c_str()) : ecoz2_mm_show(model.c_str())) printf("%s\n", e2vq_last_error());
        return 0;
    }
    if (M < 1 || sequences.empty()) return usage();
    const std::string subdir = "sequences/M" + std::to_string(M);
    std::vector<std::string> seq_files;
    if (cmd == "learn") {  // main_nbayes_learn / main_mm_learn: resolve_files(sequences, "TRAIN", class_name, ..)
        int rc = is_csv_list(sequences) ? e2vq_io::files_from_csv(sequences[0], "TRAIN", cls, subdir, ".seq", nullptr, seq_files)
                                        : e2vq_io::resolve_filenames(sequences, ".seq", seq_files);
        if (rc || seq_files.empty()) { printf("%s\n", rc ? e2vq_last_error() : "No sequences given"); return 0; }
        auto ps = cptrs(seq_files);
        if (nb ? ecoz2_nb_learn(M, ps.data(), (int)ps.size(), nullptr, 0) : ecoz2_mm_learn(M, ps.data(), (int)ps.size(), nullptr, 0))
            printf("%s\n", e2vq_last_error());
        return 0;
    }
    if (cmd == "classify") {  // main_nbayes_classify / main_mm_classify
        if (tt.empty() || models.empty()) return usage();
        std::vector<std::string> model_files;
        e2vq_io::resolve_filenames(models, ext, model_files);
        if (model_files.empty()) { printf("No models given\n"); return 0; }
        int rc = is_csv_list(sequences) ? e2vq_io::files_from_csv(sequences[0], tt, "", subdir, ".seq", nullptr, seq_files)
                                        : e2vq_io::resolve_filenames(sequences, ".seq", seq_files);
        if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
        printf("number of %s models: %zu  number of sequences: %zu\n", nb ? "NBayes" : "MM", model_files.size(), seq_files.size());
        printf("show_ranked = %s\n", ranked ? "true" : "false");
        auto pm = cptrs(model_files), ps = cptrs(seq_files);
        if (nb ? ecoz2_nb_classify(pm.data(), (int)pm.size(), ps.data(), (int)ps.size(), ranked, M)
               : ecoz2_mm_classify(pm.data(), (int)pm.size(), ps.data(), (int)ps.size(), ranked, M))
            printf("%s\n", e2vq_last_error());
        return 0;
    }
    return usage();
}

// `ecoz2 hmm {learn,classify,show}`: option structs and mains of /root/reference/src/hmm/mod.rs:40-291
static void hmm_callback(char*, double) {}  // the reference's Rust callback is a no-op too (src/hmm/mod.rs:205-207)

// "a,b,c" -> integers; false unless every item is a whole decimal integer
static bool int_list(const std::string& text, std::vector<int>& out)
{
    out.clear();
    size_t at = 0;
    for (;;) {
        const size_t end = std::min(text.find(',', at), text.size());
        const std::string item = text.substr(at, end - at);
        char* stop = nullptr;
        const long v = strtol(item.c_str(), &stop, 10);
        if (item.empty() || *stop != 0 || v < INT_MIN || v > INT_MAX) return false;
        out.push_back((int)v);
        if (end == text.size()) return true;
        at = end + 1;
    }
}

// `hmm learn --grid -N <n1,...> -M <m1,...>`: one model per (N, M, class) in one training.  With a
// tt.csv each M takes the TRAIN rows under sequences/M<m>; every file's header M must be listed and every listed M must
// have a file.
static int hmm_learn_grid(const std::string& n_arg, const std::string& m_arg, const std::string& cls, int type, int max_iterations,
                          double epsilon, double val_auto, long seed, const std::vector<std::string>& sequences)
{
    if (!cls.empty()) {
        fprintf(stderr, "--grid and --class-name exclude each other\n");
        return usage();
    }
    std::vector<int> ns, ms;
    if (!int_list(n_arg, ns) || !int_list(m_arg, ms)) {
        fprintf(stderr, "--grid needs -N <n1,n2,...> and -M <m1,m2,...>: comma-separated integers\n");
        return usage();
    }
    std::sort(ns.begin(), ns.end());
    std::sort(ms.begin(), ms.end());
    for (size_t i = 0; i < ms.size(); ++i)
        if (ms[i] < 1 || (i > 0 && ms[i] == ms[i - 1])) {
            fprintf(stderr, "-M %d: %s\n", ms[i], ms[i] < 1 ? "not a codebook size" : "given more than once");
            return usage();
        }
    std::vector<std::string> seq_files;
    int rc = 0;
    if (is_csv_list(sequences)) {
        for (int m : ms) {
            std::vector<std::string> f;
            rc = e2vq_io::files_from_csv(sequences[0], "TRAIN", "", "sequences/M" + std::to_string(m), ".seq", nullptr, f);
            if (rc) break;
            seq_files.insert(seq_files.end(), f.begin(), f.end());
        }
    } else {
        rc = e2vq_io::resolve_filenames(sequences, ".seq", seq_files);
    }
    if (rc || seq_files.empty()) { printf("%s\n", rc ? e2vq_last_error() : "No sequences given"); return 0; }
    std::set<std::string> classes;
    std::set<int> seen_M;
    for (const std::string& f : seq_files) {
        char c[96];
        int m;
        int64_t T;
        if (e2vq_seq_info(f.c_str(), c, &m, &T)) { printf("%s\n", e2vq_last_error()); return 0; }
        if (!std::binary_search(ms.begin(), ms.end(), m)) { printf("%s: codebook size %d is not in the -M list\n", f.c_str(), m); return 0; }
        classes.insert(c);
        seen_M.insert(m);
    }
    for (int m : ms)
        if (!seen_M.count(m)) { printf("no sequence with codebook size %d among the given ones\n", m); return 0; }
    auto joined = [](const std::vector<int>& v) {
        std::string s;
        for (int x : v) s += (s.empty() ? "" : ",") + std::to_string(x);
        return s;
    };
    printf("ECOZ2 C version: %s\n", ecoz2_version());
    printf("sequences: %zu\n", seq_files.size());
    printf("classes: %zu\n", classes.size());
    printf("grid: N=%s M=%s\n", joined(ns).c_str(), joined(ms).c_str());
    printf("val_auto = %g\n", val_auto);
    ecoz2_set_random_seed(seed);
    auto ps = cptrs(seq_files);
    if (e2vq_hmm_learn_grid(ns.data(), (int)ns.size(), type, ps.data(), (unsigned)ps.size(), epsilon, val_auto, max_iterations,
                            hmm_callback))
        printf("%s\n", e2vq_last_error());
    return 0;
}

// `hmm classify --grid`: every (N, M) point of the given models classified in one batched scoring.
// With a tt.csv each M of -M takes the --tt rows under sequences/M<m>; with directories or files -M, if given, filters
// both the models and the sequences by their headers.
static int hmm_classify_grid(const std::string& m_arg, const std::string& cls, const std::string& tt, bool ranked,
                             const std::string& c12n_dir, const std::string& summary, const std::vector<std::string>& models,
                             const std::vector<std::string>& sequences, const std::vector<std::string>& predictors,
                             const std::vector<std::string>& codebooks)
{
    const char* excluded = !cls.empty() ? "--class-name" : !predictors.empty() ? "--predictors" : !codebooks.empty() ? "--codebooks" : nullptr;
    if (excluded) {
        fprintf(stderr, "--grid and %s exclude each other\n", excluded);
        return usage();
    }
    if (models.empty() || tt.empty() || sequences.empty()) return usage();
    std::vector<int> ms;
    if (!m_arg.empty() && !int_list(m_arg, ms)) {
        fprintf(stderr, "--grid takes -M <m1,m2,...>: comma-separated integers\n");
        return usage();
    }
    const bool csv = is_csv_list(sequences);
    if (csv && ms.empty()) {
        fprintf(stderr, "--grid with a tt.csv needs -M <m1,m2,...>\n");
        return usage();
    }
    std::sort(ms.begin(), ms.end());
    for (size_t i = 0; i < ms.size(); ++i)
        if (ms[i] < 1 || (i > 0 && ms[i] == ms[i - 1])) {
            fprintf(stderr, "-M %d: %s\n", ms[i], ms[i] < 1 ? "not a codebook size" : "given more than once");
            return usage();
        }
    std::vector<std::string> found_models, hmm_files, found_seqs, seq_files;
    e2vq_io::resolve_filenames(models, ".hmm", found_models);
    int rc = 0;
    if (csv) {
        for (int m : ms) {
            std::vector<std::string> f;
            rc = e2vq_io::files_from_csv(sequences[0], tt, "", "sequences/M" + std::to_string(m), ".seq", nullptr, f);
            if (rc) break;
            found_seqs.insert(found_seqs.end(), f.begin(), f.end());
        }
    } else {
        rc = e2vq_io::resolve_filenames(sequences, ".seq", found_seqs);
    }
    if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
    auto listed = [&](int m) { return ms.empty() || std::binary_search(ms.begin(), ms.end(), m); };
    std::set<std::pair<int, int>> points;
    for (const std::string& f : found_models) {
        char c[96];
        int n, m;
        if (e2vq_hmm_info(f.c_str(), c, &n, &m)) { printf("%s\n", e2vq_last_error()); return 0; }
        if (!listed(m)) continue;
        hmm_files.push_back(f);
        points.insert({n, m});
    }
    for (const std::string& f : found_seqs) {
        char c[96];
        int m;
        int64_t T;
        if (e2vq_seq_info(f.c_str(), c, &m, &T)) { printf("%s\n", e2vq_last_error()); return 0; }
        if (listed(m)) seq_files.push_back(f);
    }
    if (hmm_files.empty()) { printf("No models given\n"); return 0; }
    if (seq_files.empty()) { printf("No sequences given\n"); return 0; }
    printf("ECOZ2 C version: %s\n", ecoz2_version());
    printf("number of HMM models: %zu  number of sequences: %zu\n", hmm_files.size(), seq_files.size());
    printf("grid points: %zu\n", points.size());
    printf("show_ranked = %s\n", ranked ? "true" : "false");
    auto pm = cptrs(hmm_files), ps = cptrs(seq_files);
    if (e2vq_hmm_classify_grid(pm.data(), (unsigned)pm.size(), ps.data(), (unsigned)ps.size(), ranked, c12n_dir.empty() ? nullptr : c12n_dir.c_str(),
                               summary.empty() ? nullptr : summary.c_str()))
        printf("%s\n", e2vq_last_error());
    return 0;
}

// `hmm scan`: the trained models over sliding windows of whole recordings
// the value of a flag that chooses a kernel body: auto, resident or looped; anything else is named on stderr under `prefix`
static bool body_value_ok(const char* prefix, const char* flag, const std::string& v)
{
    if (v == "auto" || v == "resident" || v == "looped") return true;
    fprintf(stderr, "%s: %s %s: auto, resident or looped\n", prefix, flag, v.c_str());
    return false;
}

static int hmm_scan_cmd(int argc, char** argv)
{
    int P = 36, W = 45, O = 15;
    long long window = 0, hop = 0;
    double min_margin = 0.0;
    std::string codebook, csv;
    std::vector<std::string> models, signals, predictors, sequences;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        auto num = [&](const char* name) -> long long {
            const char* v = val(name);
            char* end = nullptr;
            const long long x = strtoll(v, &end, 10);
            if (!*v || *end) { fprintf(stderr, "%s: invalid value '%s'\n", name, v); exit(2); }
            return x;
        };
        auto many = [&](std::vector<std::string>& v) { while (i + 1 < argc && !is_flag(argv[i + 1])) v.push_back(argv[++i]); };
        if (a == "-m" || a == "--models") many(models);
        else if (a == "--codebook") codebook = val("--codebook");
        else if (a == "-P" || a == "--prediction-order") P = (int)num("-P");
        else if (a == "-W" || a == "--window-length-ms") W = (int)num("-W");
        else if (a == "-O" || a == "--offset-length-ms") O = (int)num("-O");
        else if (a == "--window") window = num("--window");
        else if (a == "--hop") hop = num("--hop");
        else if (a == "--min-margin") min_margin = atof(val("--min-margin"));
        else if (a == "-c" || a == "--csv") csv = val("-c");
        else if (a == "--signals") many(signals);
        else if (a == "--predictors") many(predictors);
        else if (a == "-s" || a == "--sequences") many(sequences);
        else return usage();
    }
    if (models.empty()) { fprintf(stderr, "hmm scan: --models <files|dirs>... is required\n"); return usage(); }
    if ((int)!signals.empty() + (int)!predictors.empty() + (int)!sequences.empty() != 1) {
        fprintf(stderr, "hmm scan: exactly one of --signals, --predictors and --sequences is required\n");
        return usage();
    }
    if (window < 1) { fprintf(stderr, "hmm scan: --window <frames> is required and at least 1\n"); return 2; }
    if (hop == 0) hop = window;
    if (hop < 1) { fprintf(stderr, "hmm scan: --hop %lld: at least 1\n", hop); return 2; }
    if (P < 1 || P > 80) { fprintf(stderr, "-P %d: prediction order out of range [1, 80]\n", P); return 2; }
    if (O < 1 || W < 1) { fprintf(stderr, "-W and -O must be positive\n"); return 2; }
    if (sequences.empty() && codebook.empty()) { fprintf(stderr, "hmm scan: --signals and --predictors need --codebook <cbook>\n"); return 2; }
    std::vector<std::string> hmm_files, inputs;
    e2vq_io::resolve_filenames(models, ".hmm", hmm_files);
    if (hmm_files.empty()) { printf("No models given\n"); return 0; }
    const int rc = !signals.empty() ? e2vq_io::resolve_filenames(signals, ".wav", inputs)
                   : !predictors.empty() ? e2vq_io::resolve_filenames(predictors, ".prd", inputs)
                                         : e2vq_io::resolve_filenames(sequences, ".seq", inputs);
    if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
    if (inputs.empty()) { printf("No inputs given\n"); return 0; }
    printf("ECOZ2 C version: %s\n", ecoz2_version());
    printf("number of HMM models: %zu  number of inputs: %zu\n", hmm_files.size(), inputs.size());
    auto pm = cptrs(hmm_files), pi = cptrs(inputs);
    if (e2vq_hmm_scan_files(pm.data(), (unsigned)pm.size(), codebook.empty() ? nullptr : codebook.c_str(), pi.data(), (int)pi.size(), P,
                            W, O, window, hop, min_margin, csv.empty() ? nullptr : csv.c_str())) {
        printf("%s\n", e2vq_last_error());
        return 1;
    }
    return 0;
}

// `hmm segment`: each recording decoded once under the class loop of the trained models
static int hmm_segment_cmd(int argc, char** argv)
{
    int P = 36, W = 45, O = 15;
    double ln_switch = 0.0;
    bool have_switch = false;
    bool posteriors = false;
    bool continuous = false;
    bool grammar = false;  // --grammar-posteriors
    bool grammar_continuous = false;
    bool cont_post = false, have_block = false;  // --continuous-posteriors; --block or --lookahead
    long long block = 4096, lookahead = 4096;
    bool have_grammar_body = false, have_post_body = false;
    std::string codebook, csv, frames_dir, transitions, rec_name, grammar_name, post_name, body, grammar_body, post_body;
    std::vector<std::string> models, signals, predictors, sequences;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        auto num = [&](const char* name) -> long long {
            const char* v = val(name);
            char* end = nullptr;
            const long long x = strtoll(v, &end, 10);
            if (!*v || *end) { fprintf(stderr, "%s: invalid value '%s'\n", name, v); exit(2); }
            return x;
        };
        auto many = [&](std::vector<std::string>& v) { while (i + 1 < argc && !is_flag(argv[i + 1])) v.push_back(argv[++i]); };
        if (a == "-m" || a == "--models") many(models);
        else if (a == "--codebook") codebook = val("--codebook");
        else if (a == "-P" || a == "--prediction-order") P = (int)num("-P");
        else if (a == "-W" || a == "--window-length-ms") W = (int)num("-W");
        else if (a == "-O" || a == "--offset-length-ms") O = (int)num("-O");
        else if (a == "--posteriors") posteriors = true;
        else if (a == "--grammar-posteriors") grammar = true;
        else if (a == "--body") body = val("--body");
        else if (a == "--grammar-body") { grammar_body = val("--grammar-body"); have_grammar_body = true; }
        else if (a == "--grammar-posteriors-body") { post_body = val("--grammar-posteriors-body"); have_post_body = true; }
        else if (a == "--continuous") { rec_name = val("--continuous"); continuous = true; }
        else if (a == "--grammar-continuous") { grammar_name = val("--grammar-continuous"); grammar_continuous = true; }
        else if (a == "--continuous-posteriors") { post_name = val("--continuous-posteriors"); cont_post = true; }
        else if (a == "--block") { block = num("--block"); have_block = true; }
        else if (a == "--lookahead") { lookahead = num("--lookahead"); have_block = true; }
        else if (a == "--frame-posteriors") frames_dir = val("--frame-posteriors");
        else if (a == "--class-transitions") transitions = val("--class-transitions");
        else if (a == "--switch-penalty") {
            const char* v = val("--switch-penalty");
            char* end = nullptr;
            ln_switch = strtod(v, &end);
            if (!*v || *end) { fprintf(stderr, "--switch-penalty: invalid value '%s'\n", v); exit(2); }
            have_switch = true;
        }
        else if (a == "-c" || a == "--csv") csv = val("-c");
        else if (a == "--signals") many(signals);
        else if (a == "--predictors") many(predictors);
        else if (a == "-s" || a == "--sequences") many(sequences);
        else return usage();
    }
    if (models.empty()) { fprintf(stderr, "hmm segment: --models <files|dirs>... is required\n"); return usage(); }
    if ((int)!signals.empty() + (int)!predictors.empty() + (int)!sequences.empty() != 1) {
        fprintf(stderr, "hmm segment: exactly one of --signals, --predictors and --sequences is required\n");
        return usage();
    }
    if (!have_switch) { fprintf(stderr, "hmm segment: --switch-penalty <x <= 0 | -inf> is required\n"); return 2; }
    if (!(ln_switch <= 0.0)) { fprintf(stderr, "hmm segment: --switch-penalty %g: at most 0\n", ln_switch); return 2; }
    if (P < 1 || P > 80) { fprintf(stderr, "-P %d: prediction order out of range [1, 80]\n", P); return 2; }
    if (O < 1 || W < 1) { fprintf(stderr, "-W and -O must be positive\n"); return 2; }
    if (sequences.empty() && codebook.empty()) { fprintf(stderr, "hmm segment: --signals and --predictors need --codebook <cbook>\n"); return 2; }
    if (cont_post) {  // (its own refusals first: the ones below speak of the other modes)
        if (continuous || posteriors || !transitions.empty() || grammar || grammar_continuous || have_grammar_body || have_post_body) {
            fprintf(stderr, "hmm segment: --continuous-posteriors gives the posteriors of one stream under the one switch penalty: not with "
                            "--continuous, --posteriors, --class-transitions, --grammar-posteriors, --grammar-continuous, --grammar-body or "
                            "--grammar-posteriors-body\n");
            return 2;
        }
        if (post_name.empty()) { fprintf(stderr, "hmm segment: --continuous-posteriors <name>: the recording needs a name\n"); return 2; }
        if (block < 1) { fprintf(stderr, "hmm segment: --block %lld: at least 1 frame\n", block); return 2; }
        if (lookahead < 0) { fprintf(stderr, "hmm segment: --lookahead %lld: at least 0 frames\n", lookahead); return 2; }
    } else if (have_block) {
        fprintf(stderr, "hmm segment: --block and --lookahead need --continuous-posteriors <name> (they are its block and its look-ahead)\n");
        return 2;
    }
    if (have_grammar_body) {  // the body of the decoder under the prices (ECOZ2_HMM_SEGMENT_TRANS_BODY), set in this process before the call
        if (transitions.empty()) {
            fprintf(stderr, "hmm segment: --grammar-body <auto|resident|looped> needs --class-transitions <file.csv> (it chooses the body of "
                            "the decoder under its prices)\n");
            return 2;
        }
        if (grammar) {
            fprintf(stderr, "hmm segment: --grammar-posteriors has the resident body only: not with --grammar-body\n");
            return 2;
        }
        if (!body_value_ok("hmm segment --class-transitions", "--grammar-body", grammar_body)) return 2;
        setenv("ECOZ2_HMM_SEGMENT_TRANS_BODY", grammar_body.c_str(), 1);
    }
    if (have_post_body) {  // the body of the posteriors under the prices (ECOZ2_HMM_TRANS_FB_BODY), set in this process before the call
        if (!grammar) {
            fprintf(stderr, "hmm segment: --grammar-posteriors-body <auto|resident|looped> needs --grammar-posteriors (it chooses the body "
                            "of the posteriors under the prices)\n");
            return 2;
        }
        if (!body_value_ok("hmm segment --grammar-posteriors", "--grammar-posteriors-body", post_body)) return 2;
    }
    if (grammar_continuous) {  // (its own refusals first: the ones below speak of the other modes)
        if (continuous || posteriors || grammar || !frames_dir.empty() || !body.empty()) {
            fprintf(stderr, "hmm segment: --grammar-continuous decodes one stream under the prices of --class-transitions: not with "
                            "--continuous, --posteriors, --grammar-posteriors, --frame-posteriors or --body\n");
            return 2;
        }
        if (transitions.empty()) {
            fprintf(stderr, "hmm segment: --grammar-continuous needs --class-transitions <file.csv> (the stream is decoded under its prices)\n");
            return 2;
        }
        if (grammar_name.empty()) { fprintf(stderr, "hmm segment: --grammar-continuous <name>: the recording needs a name\n"); return 2; }
    }
    if (!frames_dir.empty() && !posteriors && !grammar && !cont_post) { fprintf(stderr, "hmm segment: --frame-posteriors <dir> needs --posteriors\n"); return 2; }
    if (grammar && (continuous || !body.empty())) {
        fprintf(stderr, "hmm segment: --grammar-posteriors has the resident body and whole recordings only: not with --continuous or --body\n");
        return 2;
    }
    if (!body.empty()) {  // the body of the posteriors (ECOZ2_HMM_POSTERIOR_BODY), set in this process before the call
        if (!posteriors && !cont_post) { fprintf(stderr, "hmm segment: --body <auto|resident|looped> needs --posteriors\n"); return 2; }
        if (!body_value_ok(cont_post ? "hmm segment --continuous-posteriors" : "hmm segment --posteriors", "--body", body)) return usage();
        setenv("ECOZ2_HMM_POSTERIOR_BODY", body.c_str(), 1);
    }
    if (!transitions.empty() && posteriors) {
        fprintf(stderr, "hmm segment: --class-transitions and --posteriors exclude one another (the posteriors know one price only)\n");
        return 2;
    }
    if (grammar && transitions.empty()) {
        fprintf(stderr, "hmm segment: --grammar-posteriors needs --class-transitions <file.csv> (the posteriors under its prices)\n");
        return 2;
    }
    if (continuous && (posteriors || !transitions.empty())) {
        fprintf(stderr, "hmm segment: --continuous decodes under the one switch penalty: not with --posteriors or --class-transitions\n");
        return 2;
    }
    if (continuous && rec_name.empty()) { fprintf(stderr, "hmm segment: --continuous <name>: the recording needs a name\n"); return 2; }
    if (have_post_body) setenv("ECOZ2_HMM_TRANS_FB_BODY", post_body.c_str(), 1);
    std::vector<std::string> hmm_files, inputs;
    e2vq_io::resolve_filenames(models, ".hmm", hmm_files);
    if (hmm_files.empty()) { printf("No models given\n"); return 0; }
    const int rc = !signals.empty() ? e2vq_io::resolve_filenames(signals, ".wav", inputs)
                   : !predictors.empty() ? e2vq_io::resolve_filenames(predictors, ".prd", inputs)
                                         : e2vq_io::resolve_filenames(sequences, ".seq", inputs);
    if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
    if (inputs.empty()) { printf("No inputs given\n"); return 0; }
    printf("ECOZ2 C version: %s\n", ecoz2_version());
    printf("number of HMM models: %zu  number of inputs: %zu\n", hmm_files.size(), inputs.size());
    auto pm = cptrs(hmm_files), pi = cptrs(inputs);
    const char* cb = codebook.empty() ? nullptr : codebook.c_str();
    const char* out = csv.empty() ? nullptr : csv.c_str();
    const int failed = cont_post
                           ? e2vq_hmm_segment_continuous_files_posteriors(pm.data(), (unsigned)pm.size(), cb, pi.data(), (int)pi.size(), P, W, O,
                                                                          ln_switch, post_name.c_str(), out,
                                                                          frames_dir.empty() ? nullptr : frames_dir.c_str(), block, lookahead)
                       : grammar_continuous
                           ? e2vq_hmm_segment_trans_continuous_files(pm.data(), (unsigned)pm.size(), cb, pi.data(), (int)pi.size(), P, W, O, ln_switch,
                                                                     transitions.c_str(), grammar_name.c_str(), out)
                       : continuous ? e2vq_hmm_segment_continuous_files(pm.data(), (unsigned)pm.size(), cb, pi.data(), (int)pi.size(), P, W, O,
                                                                      ln_switch, rec_name.c_str(), out)
                       : grammar ? e2vq_hmm_segment_trans_files_posteriors(pm.data(), (unsigned)pm.size(), cb, pi.data(), (int)pi.size(), P, W, O,
                                                                           ln_switch, transitions.c_str(), out,
                                                                           frames_dir.empty() ? nullptr : frames_dir.c_str())
                       : !transitions.empty() ? e2vq_hmm_segment_trans_files(pm.data(), (unsigned)pm.size(), cb, pi.data(), (int)pi.size(), P, W, O,
                                                                           ln_switch, transitions.c_str(), out)
                       : posteriors ? e2vq_hmm_segment_files_posteriors(pm.data(), (unsigned)pm.size(), cb, pi.data(), (int)pi.size(), P, W, O,
                                                                      ln_switch, out, frames_dir.empty() ? nullptr : frames_dir.c_str())
                                  : e2vq_hmm_segment_files(pm.data(), (unsigned)pm.size(), cb, pi.data(), (int)pi.size(), P, W, O, ln_switch, out);
    if (failed) {
        printf("%s\n", e2vq_last_error());
        return 1;
    }
    return 0;
}

// `hmm transitions --em`: the same matrix by Baum-Welch from unlabelled recordings under the trained models
static int hmm_transitions_em_cmd(int argc, char** argv)
{
    int P = 36, W = 45, O = 15, max_iterations = -1;
    double ln_switch = 0.0, alpha = 1.0, val_auto = 0.3;
    bool have_switch = false, have_body = false;
    std::string codebook, init, out, body;
    std::vector<std::string> models, signals, predictors, sequences;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        auto num = [&](const char* name) -> long long {
            const char* v = val(name);
            char* end = nullptr;
            const long long x = strtoll(v, &end, 10);
            if (!*v || *end) { fprintf(stderr, "%s: invalid value '%s'\n", name, v); exit(2); }
            return x;
        };
        auto real = [&](const char* name) -> double {
            const char* v = val(name);
            char* end = nullptr;
            const double x = strtod(v, &end);
            if (!*v || *end) { fprintf(stderr, "%s: invalid value '%s'\n", name, v); exit(2); }
            return x;
        };
        auto many = [&](std::vector<std::string>& v) { while (i + 1 < argc && !is_flag(argv[i + 1])) v.push_back(argv[++i]); };
        if (a == "--em") continue;
        else if (a == "-m" || a == "--models") many(models);
        else if (a == "--codebook") codebook = val("--codebook");
        else if (a == "-P" || a == "--prediction-order") P = (int)num("-P");
        else if (a == "-W" || a == "--window-length-ms") W = (int)num("-W");
        else if (a == "-O" || a == "--offset-length-ms") O = (int)num("-O");
        else if (a == "--switch-penalty") { ln_switch = real("--switch-penalty"); have_switch = true; }
        else if (a == "--init") init = val("--init");
        else if (a == "--alpha") alpha = real("--alpha");
        else if (a == "-a") val_auto = real("-a");
        else if (a == "-I") max_iterations = (int)num("-I");
        else if (a == "-o" || a == "--output") out = val("-o");
        else if (a == "--body") { body = val("--body"); have_body = true; }
        else if (a == "--signals") many(signals);
        else if (a == "--predictors") many(predictors);
        else if (a == "--sequences") many(sequences);
        else return usage();
    }
    if (have_body) {  // the E-step's body (ECOZ2_HMM_TRANS_FB_BODY), set in this process before the call
        if (!body_value_ok("hmm transitions --em", "--body", body)) return 2;
        setenv("ECOZ2_HMM_TRANS_FB_BODY", body.c_str(), 1);
    }
    if (models.empty()) { fprintf(stderr, "hmm transitions --em: --models <files|dirs>... is required\n"); return usage(); }
    if ((int)!signals.empty() + (int)!predictors.empty() + (int)!sequences.empty() != 1) {
        fprintf(stderr, "hmm transitions --em: exactly one of --signals, --predictors and --sequences is required\n");
        return usage();
    }
    if (!have_switch) { fprintf(stderr, "hmm transitions --em: --switch-penalty <x <= 0 | -inf> is required\n"); return 2; }
    if (!(ln_switch <= 0.0)) { fprintf(stderr, "hmm transitions --em: --switch-penalty %g: at most 0\n", ln_switch); return 2; }
    if (out.empty()) { fprintf(stderr, "hmm transitions --em: -o <file.csv> is required\n"); return 2; }
    if (!(alpha >= 0.0)) { fprintf(stderr, "hmm transitions --em: --alpha %g: at least 0\n", alpha); return 2; }
    if (P < 1 || P > 80) { fprintf(stderr, "-P %d: prediction order out of range [1, 80]\n", P); return 2; }
    if (O < 1 || W < 1) { fprintf(stderr, "-W and -O must be positive\n"); return 2; }
    if (sequences.empty() && codebook.empty()) { fprintf(stderr, "hmm transitions --em: --signals and --predictors need --codebook <cbook>\n"); return 2; }
    std::vector<std::string> hmm_files, inputs;
    e2vq_io::resolve_filenames(models, ".hmm", hmm_files);
    if (hmm_files.empty()) { printf("No models given\n"); return 0; }
    const int rc = !signals.empty() ? e2vq_io::resolve_filenames(signals, ".wav", inputs)
                   : !predictors.empty() ? e2vq_io::resolve_filenames(predictors, ".prd", inputs)
                                         : e2vq_io::resolve_filenames(sequences, ".seq", inputs);
    if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
    if (inputs.empty()) { printf("No inputs given\n"); return 0; }
    printf("ECOZ2 C version: %s\n", ecoz2_version());
    printf("number of HMM models: %zu  number of inputs: %zu\n", hmm_files.size(), inputs.size());
    auto pm = cptrs(hmm_files), pi = cptrs(inputs);
    if (e2vq_hmm_learn_transitions_files(pm.data(), (unsigned)pm.size(), codebook.empty() ? nullptr : codebook.c_str(), pi.data(),
                                         (int)pi.size(), P, W, O, ln_switch, init.empty() ? nullptr : init.c_str(), alpha, val_auto,
                                         max_iterations, out.c_str())) {
        printf("%s\n", e2vq_last_error());
        return 1;
    }
    return 0;
}

// `hmm transitions`: the class-to-class prices of `hmm segment --class-transitions` from labelled successions
static int hmm_transitions_cmd(int argc, char** argv)
{
    for (int i = 0; i < argc; ++i)
        if (strcmp(argv[i], "--em") == 0) return hmm_transitions_em_cmd(argc, argv);
    double alpha = 1.0;
    std::string out;
    std::vector<std::string> models, inputs;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        if (a == "-m" || a == "--models") { while (i + 1 < argc && !is_flag(argv[i + 1])) models.push_back(argv[++i]); }
        else if (a == "--alpha") {
            const char* v = val("--alpha");
            char* end = nullptr;
            alpha = strtod(v, &end);
            if (!*v || *end) { fprintf(stderr, "--alpha: invalid value '%s'\n", v); exit(2); }
        }
        else if (a == "-o" || a == "--output") out = val("-o");
        else if (a == "--init" || a == "-a" || a == "-I" || a == "--body" || a == "--sequences" || a == "--predictors" || a == "--signals") {
            fprintf(stderr, "hmm transitions: %s needs --em (the matrix from unlabelled recordings)\n", a.c_str());
            return 2;
        }
        else if (is_flag(argv[i])) return usage();
        else inputs.push_back(a);
    }
    if (models.empty()) { fprintf(stderr, "hmm transitions: --models <files|dirs>... is required\n"); return usage(); }
    if (out.empty()) { fprintf(stderr, "hmm transitions: -o <file.csv> is required\n"); return 2; }
    if (!(alpha >= 0.0)) { fprintf(stderr, "hmm transitions: --alpha %g: at least 0\n", alpha); return 2; }
    if (inputs.empty()) { fprintf(stderr, "hmm transitions: no inputs\n"); return 2; }
    std::vector<std::string> hmm_files;
    e2vq_io::resolve_filenames(models, ".hmm", hmm_files);
    if (hmm_files.empty()) { printf("No models given\n"); return 0; }
    auto pm = cptrs(hmm_files), pi = cptrs(inputs);
    if (e2vq_hmm_transitions_files(pm.data(), (unsigned)pm.size(), pi.data(), (int)pi.size(), alpha, out.c_str())) {
        printf("%s\n", e2vq_last_error());
        return 1;
    }
    return 0;
}

// `hmm align`: each recording aligned to the known order of its units under the trained models
static int hmm_align_cmd(int argc, char** argv)
{
    int P = 36, W = 45, O = 15;
    double ln_switch = 0.0;
    bool posteriors = false, have_body = false;
    std::string codebook, csv, filler, frames_dir, body;
    std::vector<std::string> models, labels, signals, predictors, sequences;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        auto num = [&](const char* name) -> long long {
            const char* v = val(name);
            char* end = nullptr;
            const long long x = strtoll(v, &end, 10);
            if (!*v || *end) { fprintf(stderr, "%s: invalid value '%s'\n", name, v); exit(2); }
            return x;
        };
        auto many = [&](std::vector<std::string>& v) { while (i + 1 < argc && !is_flag(argv[i + 1])) v.push_back(argv[++i]); };
        if (a == "-m" || a == "--models") many(models);
        else if (a == "--codebook") codebook = val("--codebook");
        else if (a == "-P" || a == "--prediction-order") P = (int)num("-P");
        else if (a == "-W" || a == "--window-length-ms") W = (int)num("-W");
        else if (a == "-O" || a == "--offset-length-ms") O = (int)num("-O");
        else if (a == "--filler") filler = val("--filler");
        else if (a == "--labels") many(labels);
        else if (a == "--switch-penalty") {
            const char* v = val("--switch-penalty");
            char* end = nullptr;
            ln_switch = strtod(v, &end);
            if (!*v || *end) { fprintf(stderr, "--switch-penalty: invalid value '%s'\n", v); exit(2); }
        }
        else if (a == "-c" || a == "--csv") csv = val("-c");
        else if (a == "--posteriors") posteriors = true;
        else if (a == "--frame-posteriors") frames_dir = val("--frame-posteriors");
        else if (a == "--body") { body = val("--body"); have_body = true; }
        else if (a == "--signals") many(signals);
        else if (a == "--predictors") many(predictors);
        else if (a == "-s" || a == "--sequences") many(sequences);
        else return usage();
    }
    if (models.empty()) { fprintf(stderr, "hmm align: --models <files|dirs>... is required\n"); return usage(); }
    if ((int)!signals.empty() + (int)!predictors.empty() + (int)!sequences.empty() != 1) {
        fprintf(stderr, "hmm align: exactly one of --signals, --predictors and --sequences is required\n");
        return usage();
    }
    if (!(ln_switch <= 0.0) || std::isinf(ln_switch)) { fprintf(stderr, "hmm align: --switch-penalty %g: finite and at most 0\n", ln_switch); return 2; }
    if (!frames_dir.empty() && !posteriors) { fprintf(stderr, "hmm align: --frame-posteriors <dir> needs --posteriors\n"); return 2; }
    if (have_body) {  // the body of the posteriors (ECOZ2_HMM_ALIGN_POSTERIOR_BODY), set in this process before the call
        if (!posteriors) {
            fprintf(stderr, "hmm align: --body <auto|resident|looped> needs --posteriors (it chooses the body of the posteriors; the "
                            "alignment picks its own)\n");
            return 2;
        }
        if (!body_value_ok("hmm align --posteriors", "--body", body)) return 2;
        setenv("ECOZ2_HMM_ALIGN_POSTERIOR_BODY", body.c_str(), 1);
    }
    if (P < 1 || P > 80) { fprintf(stderr, "-P %d: prediction order out of range [1, 80]\n", P); return 2; }
    if (O < 1 || W < 1) { fprintf(stderr, "-W and -O must be positive\n"); return 2; }
    if (sequences.empty() && codebook.empty()) { fprintf(stderr, "hmm align: --signals and --predictors need --codebook <cbook>\n"); return 2; }
    // (the inputs are taken as given, not resolved from directories: input i goes with label file i)
    const std::vector<std::string>& inputs = !signals.empty() ? signals : !predictors.empty() ? predictors : sequences;
    if (labels.size() != inputs.size()) {
        fprintf(stderr, "hmm align: %zu label files for %zu inputs (--labels names one per input, in the inputs' order)\n", labels.size(), inputs.size());
        return 2;
    }
    std::vector<std::string> hmm_files;
    e2vq_io::resolve_filenames(models, ".hmm", hmm_files);
    if (hmm_files.empty()) { printf("No models given\n"); return 0; }
    printf("ECOZ2 C version: %s\n", ecoz2_version());
    printf("number of HMM models: %zu  number of inputs: %zu\n", hmm_files.size(), inputs.size());
    auto pm = cptrs(hmm_files), pi = cptrs(inputs), pl = cptrs(labels);
    const char *cb = codebook.empty() ? nullptr : codebook.c_str(), *fl = filler.empty() ? nullptr : filler.c_str();
    const char* out = csv.empty() ? nullptr : csv.c_str();
    if (posteriors ? e2vq_hmm_align_files_posteriors(pm.data(), (unsigned)pm.size(), cb, pi.data(), pl.data(), (int)pi.size(), P, W, O, ln_switch,
                                                     fl, out, frames_dir.empty() ? nullptr : frames_dir.c_str())
                   : e2vq_hmm_align_files(pm.data(), (unsigned)pm.size(), cb, pi.data(), pl.data(), (int)pi.size(), P, W, O, ln_switch, fl, out)) {
        printf("%s\n", e2vq_last_error());
        return 1;
    }
    return 0;
}

// `hmm learn --embedded`: the class models re-estimated from whole recordings and their transcripts
static int hmm_learn_embedded_cmd(int argc, char** argv)
{
    int P = 36, W = 45, O = 15, max_iterations = -1;
    double ln_switch = 0.0, epsilon = 1e-05, val_auto = 0.3;
    std::string codebook, filler, out, body;
    std::vector<std::string> models, labels, signals, predictors, sequences;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        auto num = [&](const char* name) -> long long {
            const char* v = val(name);
            char* end = nullptr;
            const long long x = strtoll(v, &end, 10);
            if (!*v || *end) { fprintf(stderr, "%s: invalid value '%s'\n", name, v); exit(2); }
            return x;
        };
        auto real = [&](const char* name) -> double {
            const char* v = val(name);
            char* end = nullptr;
            const double x = strtod(v, &end);
            if (!*v || *end) { fprintf(stderr, "%s: invalid value '%s'\n", name, v); exit(2); }
            return x;
        };
        auto many = [&](std::vector<std::string>& v) { while (i + 1 < argc && !is_flag(argv[i + 1])) v.push_back(argv[++i]); };
        if (a == "--embedded") continue;
        else if (a == "--all-classes" || a == "--grid" || a == "--class-name") {
            fprintf(stderr, "hmm learn --embedded excludes %s (it re-estimates the models given with --models)\n", a.c_str());
            return usage();
        }
        else if (a == "-m" || a == "--models") many(models);
        else if (a == "--codebook") codebook = val("--codebook");
        else if (a == "-P" || a == "--prediction-order") P = (int)num("-P");
        else if (a == "-W" || a == "--window-length-ms") W = (int)num("-W");
        else if (a == "-O" || a == "--offset-length-ms") O = (int)num("-O");
        else if (a == "-I" || a == "--max-iterations") max_iterations = (int)num("-I");
        else if (a == "-e") epsilon = real("-e");
        else if (a == "-a") val_auto = real("-a");
        else if (a == "--filler") filler = val("--filler");
        else if (a == "--labels") many(labels);
        else if (a == "--switch-penalty") ln_switch = real("--switch-penalty");
        else if (a == "--body") body = val("--body");
        else if (a == "-o" || a == "--out") out = val("-o");
        else if (a == "--signals") many(signals);
        else if (a == "--predictors") many(predictors);
        else if (a == "-s" || a == "--sequences") many(sequences);
        else return usage();
    }
    if (!body.empty()) {  // the E-step's body (ECOZ2_HMM_EMBED_BODY), set in this process before the call
        if (!body_value_ok("hmm learn --embedded", "--body", body)) return usage();
        setenv("ECOZ2_HMM_EMBED_BODY", body.c_str(), 1);
    }
    if (models.empty()) { fprintf(stderr, "hmm learn --embedded: --models <files|dirs>... is required\n"); return usage(); }
    if (out.empty()) { fprintf(stderr, "hmm learn --embedded: -o <dir> is required\n"); return usage(); }
    if ((int)!signals.empty() + (int)!predictors.empty() + (int)!sequences.empty() != 1) {
        fprintf(stderr, "hmm learn --embedded: exactly one of --signals, --predictors and --sequences is required\n");
        return usage();
    }
    if (!(ln_switch <= 0.0) || std::isinf(ln_switch)) { fprintf(stderr, "hmm learn --embedded: --switch-penalty %g: finite and at most 0\n", ln_switch); return 2; }
    if (P < 1 || P > 80) { fprintf(stderr, "-P %d: prediction order out of range [1, 80]\n", P); return 2; }
    if (O < 1 || W < 1) { fprintf(stderr, "-W and -O must be positive\n"); return 2; }
    if (sequences.empty() && codebook.empty()) { fprintf(stderr, "hmm learn --embedded: --signals and --predictors need --codebook <cbook>\n"); return 2; }
    // (the inputs are taken as given, not resolved from directories: input i goes with label file i)
    const std::vector<std::string>& inputs = !signals.empty() ? signals : !predictors.empty() ? predictors : sequences;
    if (labels.size() != inputs.size()) {
        fprintf(stderr, "hmm learn --embedded: %zu label files for %zu inputs (--labels names one per input, in the inputs' order)\n", labels.size(),
                inputs.size());
        return 2;
    }
    std::vector<std::string> hmm_files;
    e2vq_io::resolve_filenames(models, ".hmm", hmm_files);
    if (hmm_files.empty()) { printf("No models given\n"); return 0; }
    printf("ECOZ2 C version: %s\n", ecoz2_version());
    printf("number of HMM models: %zu  number of inputs: %zu\n", hmm_files.size(), inputs.size());
    printf("val_auto = %g\n", val_auto);
    auto pm = cptrs(hmm_files), pi = cptrs(inputs), pl = cptrs(labels);
    if (e2vq_hmm_learn_embedded_files(pm.data(), (unsigned)pm.size(), codebook.empty() ? nullptr : codebook.c_str(), pi.data(), pl.data(),
                                      (int)pi.size(), P, W, O, ln_switch, filler.empty() ? nullptr : filler.c_str(), epsilon, val_auto,
                                      max_iterations, out.c_str(), hmm_callback)) {
        printf("%s\n", e2vq_last_error());
        return 1;
    }
    return 0;
}

// `hmm learn --loop`: the class models re-estimated from whole unlabelled recordings under the class loop
static int hmm_learn_loop_cmd(int argc, char** argv)
{
    int P = 36, W = 45, O = 15, max_iterations = -1;
    double ln_switch = 0.0, alpha = 1.0, epsilon = 1e-05, val_auto = 0.3;
    bool have_switch = false, have_alpha = false, train_transitions = false;
    std::string codebook, transitions, out;
    std::vector<std::string> models, frozen, signals, predictors, sequences;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        auto num = [&](const char* name) -> long long {
            const char* v = val(name);
            char* end = nullptr;
            const long long x = strtoll(v, &end, 10);
            if (!*v || *end) { fprintf(stderr, "%s: invalid value '%s'\n", name, v); exit(2); }
            return x;
        };
        auto real = [&](const char* name) -> double {
            const char* v = val(name);
            char* end = nullptr;
            const double x = strtod(v, &end);
            if (!*v || *end) { fprintf(stderr, "%s: invalid value '%s'\n", name, v); exit(2); }
            return x;
        };
        auto many = [&](std::vector<std::string>& v) { while (i + 1 < argc && !is_flag(argv[i + 1])) v.push_back(argv[++i]); };
        if (a == "--loop") continue;
        else if (a == "--embedded" || a == "--labels" || a == "--filler" || a == "--all-classes" || a == "--grid" || a == "--class-name") {
            fprintf(stderr, "hmm learn --loop excludes %s (it re-estimates the models given with --models from unlabelled recordings)\n", a.c_str());
            return usage();
        }
        else if (a == "-m" || a == "--models") many(models);
        else if (a == "--codebook") codebook = val("--codebook");
        else if (a == "-P" || a == "--prediction-order") P = (int)num("-P");
        else if (a == "-W" || a == "--window-length-ms") W = (int)num("-W");
        else if (a == "-O" || a == "--offset-length-ms") O = (int)num("-O");
        else if (a == "-I" || a == "--max-iterations") max_iterations = (int)num("-I");
        else if (a == "-e") epsilon = real("-e");
        else if (a == "-a") val_auto = real("-a");
        else if (a == "--switch-penalty") { ln_switch = real("--switch-penalty"); have_switch = true; }
        else if (a == "--class-transitions") transitions = val("--class-transitions");
        else if (a == "--train-transitions") train_transitions = true;
        else if (a == "--alpha") { alpha = real("--alpha"); have_alpha = true; }
        else if (a == "--freeze") frozen.push_back(val("--freeze"));
        else if (a == "-o" || a == "--out") out = val("-o");
        else if (a == "--signals") many(signals);
        else if (a == "--predictors") many(predictors);
        else if (a == "-s" || a == "--sequences") many(sequences);
        else return usage();
    }
    if (models.empty()) { fprintf(stderr, "hmm learn --loop: --models <files|dirs>... is required\n"); return usage(); }
    if ((int)!signals.empty() + (int)!predictors.empty() + (int)!sequences.empty() != 1) {
        fprintf(stderr, "hmm learn --loop: exactly one of --signals, --predictors and --sequences is required\n");
        return usage();
    }
    if (!have_switch) { fprintf(stderr, "hmm learn --loop: --switch-penalty <x <= 0 | -inf> is required\n"); return 2; }
    if (!(ln_switch <= 0.0)) { fprintf(stderr, "hmm learn --loop: --switch-penalty %g: at most 0\n", ln_switch); return 2; }
    if (out.empty()) { fprintf(stderr, "hmm learn --loop: -o <dir> is required\n"); return 2; }
    if (have_alpha && !train_transitions) { fprintf(stderr, "hmm learn --loop: --alpha needs --train-transitions\n"); return 2; }
    if (!(alpha >= 0.0)) { fprintf(stderr, "hmm learn --loop: --alpha %g: at least 0\n", alpha); return 2; }
    if (!(epsilon >= 0.0)) { fprintf(stderr, "hmm learn --loop: -e %g: at least 0\n", epsilon); return 2; }
    if (P < 1 || P > 80) { fprintf(stderr, "-P %d: prediction order out of range [1, 80]\n", P); return 2; }
    if (O < 1 || W < 1) { fprintf(stderr, "-W and -O must be positive\n"); return 2; }
    if (sequences.empty() && codebook.empty()) { fprintf(stderr, "hmm learn --loop: --signals and --predictors need --codebook <cbook>\n"); return 2; }
    std::vector<std::string> hmm_files, inputs;
    e2vq_io::resolve_filenames(models, ".hmm", hmm_files);
    if (hmm_files.empty()) { printf("No models given\n"); return 0; }
    const int rc = !signals.empty() ? e2vq_io::resolve_filenames(signals, ".wav", inputs)
                   : !predictors.empty() ? e2vq_io::resolve_filenames(predictors, ".prd", inputs)
                                         : e2vq_io::resolve_filenames(sequences, ".seq", inputs);
    if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
    if (inputs.empty()) { printf("No inputs given\n"); return 0; }
    printf("ECOZ2 C version: %s\n", ecoz2_version());
    printf("number of HMM models: %zu  number of inputs: %zu\n", hmm_files.size(), inputs.size());
    printf("val_auto = %g\n", val_auto);
    auto pm = cptrs(hmm_files), pi = cptrs(inputs), pf = cptrs(frozen);
    if (e2vq_hmm_learn_loop_files(pm.data(), (unsigned)pm.size(), codebook.empty() ? nullptr : codebook.c_str(), pi.data(), (int)pi.size(), P, W,
                                  O, ln_switch, transitions.empty() ? nullptr : transitions.c_str(), train_transitions ? 1 : 0,
                                  pf.empty() ? nullptr : pf.data(), (int)pf.size(), alpha, epsilon, val_auto, max_iterations, out.c_str(),
                                  hmm_callback)) {
        printf("%s\n", e2vq_last_error());
        return 1;
    }
    return 0;
}

static int hmm_cmd(int argc, char** argv)
{
    if (argc < 1) return usage();
    const std::string cmd = argv[0];
    if (cmd == "learn") {
        for (int i = 1; i < argc; ++i)
            if (std::string(argv[i]) == "--loop") return hmm_learn_loop_cmd(argc - 1, argv + 1);
        for (int i = 1; i < argc; ++i)
            if (std::string(argv[i]) == "--train-transitions" || std::string(argv[i]) == "--freeze") {
                fprintf(stderr, "hmm learn: %s needs --loop (the models re-estimated under the class loop)\n", argv[i]);
                return 2;
            }
    }
    if (cmd == "learn")
        for (int i = 1; i < argc; ++i)
            if (std::string(argv[i]) == "--embedded") return hmm_learn_embedded_cmd(argc - 1, argv + 1);
    if (cmd == "scan") return hmm_scan_cmd(argc - 1, argv + 1);
    if (cmd == "transitions") return hmm_transitions_cmd(argc - 1, argv + 1);
    if (cmd == "segment") return hmm_segment_cmd(argc - 1, argv + 1);
    if (cmd == "align") return hmm_align_cmd(argc - 1, argv + 1);
    int N = 5, M = -1, type = 3, max_iterations = -1;
    double epsilon = 1e-05, val_auto = 0.3;
    long seed = -1;
    bool ser = false, ranked = false, all_classes = false, grid = false;
    std::string cls, tt, c12n, hmm, format = "%Lg ", tmpl = "data/predictors", n_arg, m_arg, summary;
    std::vector<std::string> sequences, models, predictors, codebooks;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        auto many = [&](std::vector<std::string>& v) { while (i + 1 < argc && !is_flag(argv[i + 1])) v.push_back(argv[++i]); };
        if (a == "-N" || a == "--num-states") N = atoi((n_arg = val("-N")).c_str());
        else if (a == "-M" || a == "--codebook-size") M = atoi((m_arg = val("-M")).c_str());
        else if (a == "-t") type = atoi(val("-t"));
        else if (a == "-I" || a == "--max-iterations") max_iterations = atoi(val("-I"));
        else if (a == "-e") epsilon = atof(val("-e"));
        else if (a == "-a") val_auto = atof(val("-a"));
        else if (cmd == "learn" && (a == "-s" || a == "--seed")) seed = atol(val("-s"));
        else if (a == "--ser") ser = true;
        else if (cmd == "learn" && a == "--all-classes") all_classes = true;
        else if ((cmd == "learn" || cmd == "classify") && a == "--grid") grid = true;
        else if (cmd == "classify" && a == "--summary") summary = val("--summary");
        else if (a == "--class-name") cls = val("--class-name");
        else if (a == "-r" || a == "--show-ranked") ranked = true;
        else if (a == "-c" || a == "--c12n") c12n = val("--c12n");
        else if (a == "--tt") tt = val("--tt");
        else if (a == "-m" || a == "--models") many(models);
        else if (a == "-s" || a == "--sequences") many(sequences);
        else if (a == "--predictors") many(predictors);
        else if (a == "--predictors-dir-template") tmpl = val("--predictors-dir-template");
        else if (a == "--codebooks") many(codebooks);
        else if (a == "--hmm") hmm = val("--hmm");
        else if (a == "-f" || a == "--format") format = val("--format");
        else if (!is_flag(argv[i])) sequences.push_back(a);
        else return usage();
    }
    if (cmd == "show") {  // main_hmm_show
        if (hmm.empty()) return usage();
        printf("hmm_show: hmm_filename=%s format=%s\n", hmm.c_str(), format.c_str());  // src/ecoz2_lib/mod.rs:482-486
        if (ecoz2_hmm_show(hmm.c_str(), format.c_str())) printf("%s\n", e2vq_last_error());
        return 0;
    }
    if (cmd == "learn" && grid) return hmm_learn_grid(n_arg.empty() ? "5" : n_arg, m_arg, cls, type, max_iterations, epsilon,
                                                      val_auto, seed, sequences);
    if (cmd == "classify" && grid) return hmm_classify_grid(m_arg, cls, tt, ranked, c12n, summary, models, sequences, predictors, codebooks);
    if (M < 1) return usage();
    const std::string subdir = "sequences/M" + std::to_string(M);
    if (cmd == "learn" && all_classes) {  // every class of the TRAIN rows / given files at once
        if (!cls.empty()) {
            fprintf(stderr, "--all-classes and --class-name exclude each other\n");
            return usage();
        }
        std::vector<std::string> seq_files;
        int rc = is_csv_list(sequences) ? e2vq_io::files_from_csv(sequences[0], "TRAIN", "", subdir, ".seq", nullptr, seq_files)
                                        : e2vq_io::resolve_filenames(sequences, ".seq", seq_files);
        if (rc || seq_files.empty()) { printf("%s\n", rc ? e2vq_last_error() : "No sequences given"); return 0; }
        std::set<std::string> classes;
        for (const std::string& f : seq_files) {
            char c[96];
            int m;
            int64_t T;
            if (e2vq_seq_info(f.c_str(), c, &m, &T)) { printf("%s\n", e2vq_last_error()); return 0; }
            classes.insert(c);
        }
        printf("ECOZ2 C version: %s\n", ecoz2_version());
        printf("sequences: %zu\n", seq_files.size());
        printf("classes: %zu\n", classes.size());
        printf("val_auto = %g\n", val_auto);
        ecoz2_set_random_seed(seed);
        auto ps = cptrs(seq_files);
        if (e2vq_hmm_learn_classes(N, type, ps.data(), (unsigned)ps.size(), epsilon, val_auto, max_iterations, hmm_callback))
            printf("%s\n", e2vq_last_error());
        return 0;
    }
    if (cmd == "learn") {  // main_hmm_learn, src/hmm/mod.rs:172-217
        std::vector<std::string> seq_files;
        int rc = is_csv_list(sequences) ? e2vq_io::files_from_csv(sequences[0], "TRAIN", cls, subdir, ".seq", nullptr, seq_files)
                                        : e2vq_io::resolve_filenames(sequences, ".seq", seq_files);
        if (rc || seq_files.empty()) { printf("%s\n", rc ? e2vq_last_error() : "No sequences given"); return 0; }
        printf("ECOZ2 C version: %s\n", ecoz2_version());
        printf("sequences: %zu\n", seq_files.size());
        printf("val_auto = %g\n", val_auto);
        ecoz2_set_random_seed(seed);
        auto ps = cptrs(seq_files);
        if (ecoz2_hmm_learn(N, type, ps.data(), (unsigned)ps.size(), epsilon, val_auto, max_iterations, ser ? 0 : 1, hmm_callback))
            printf("%s\n", e2vq_last_error());
        return 0;
    }
    if (cmd == "classify") {  // main_hmm_classify, src/hmm/mod.rs:219-283
        if (models.empty() || tt.empty() || (predictors.empty() == sequences.empty())) return usage();
        std::vector<std::string> hmm_files;
        e2vq_io::resolve_filenames(models, ".hmm", hmm_files);
        if (hmm_files.empty()) { printf("No models given\n"); return 0; }
        auto pm = cptrs(hmm_files);
        const char* c12n_file = c12n.empty() ? nullptr : c12n.c_str();
        if (!sequences.empty()) {
            std::vector<std::string> seq_files;
            int rc = is_csv_list(sequences) ? e2vq_io::files_from_csv(sequences[0], tt, cls, subdir, ".seq", nullptr, seq_files)
                                            : e2vq_io::resolve_filenames(sequences, ".seq", seq_files);
            if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
            printf("ECOZ2 C version: %s\n", ecoz2_version());
            printf("number of HMM models: %zu  number of sequences: %zu\n", hmm_files.size(), seq_files.size());
            printf("show_ranked = %s\n", ranked ? "true" : "false");
            auto ps = cptrs(seq_files);
            if (ecoz2_hmm_classify(pm.data(), (unsigned)pm.size(), ps.data(), (unsigned)ps.size(), ranked, c12n_file))
                printf("%s\n", e2vq_last_error());
        } else {
            if (codebooks.empty()) return usage();
            std::vector<std::string> cb_files, prd_files;
            e2vq_io::resolve_filenames(codebooks, ".cbook", cb_files);
            if (cb_files.empty()) { printf("No codebooks given\n"); return 0; }
            int rc = is_csv_list(predictors) ? e2vq_io::files_from_csv(predictors[0], tt, cls, "", ".prd", &tmpl, prd_files)
                                             : e2vq_io::resolve_filenames(predictors, ".prd", prd_files);
            if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
            auto pc = cptrs(cb_files), pp = cptrs(prd_files);
            if (ecoz2_hmm_classify_predictors(pm.data(), (unsigned)pm.size(), pc.data(), (int)pc.size(), pp.data(), (int)pp.size(),
                                              ranked, c12n_file))
                printf("%s\n", e2vq_last_error());
        }
        return 0;
    }
    return usage();
}

// `ecoz2 lpc`: LpcOpts and main_lpc of src/lpc/mod.rs:17-74, 87-143
static int lpc_cmd(int argc, char** argv)
{
    int P = 36, W = 45, O = 15, minpc = 0;
    float split = 0.f, mintrpt = 5.f;
    bool verbose = false;
    std::string tmpl = "data/signals", tt, cls;
    std::vector<std::string> signals;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        auto num = [&](const char* name) -> long {
            const char* v = val(name);
            char* end = nullptr;
            const long x = strtol(v, &end, 10);
            if (!*v || *end || x < 0 || x > 1000000) { fprintf(stderr, "%s: invalid value '%s'\n", name, v); exit(2); }
            return x;
        };
        auto real = [&](const char* name) -> float {
            const char* v = val(name);
            char* end = nullptr;
            const float x = strtof(v, &end);
            if (!*v || *end) { fprintf(stderr, "%s: invalid value '%s'\n", name, v); exit(2); }
            return x;
        };
        if (a == "-P" || a == "--prediction-order") P = (int)num("-P");
        else if (a == "-W" || a == "--window-length-ms") W = (int)num("-W");
        else if (a == "-O" || a == "--offset-length-ms") O = (int)num("-O");
        else if (a == "-m" || a == "--minpc") minpc = (int)num("-m");
        else if (a == "-s" || a == "--split") split = real("-s");
        else if (a == "-X") mintrpt = real("-X");
        else if (a == "--verbose") verbose = true;
        else if (a == "--signals-dir-template") tmpl = val("--signals-dir-template");
        else if (a == "--tt") tt = val("--tt");
        else if (a == "--class") cls = val("--class");
        else if (a == "--zrs" || a == "--zrsp") {
            fprintf(stderr, "%s selects the reference's Rust variants, which write CBOR predictor files; not supported "
                            "by this build (the default analysis writes the .prd format)\n",
                    a.c_str());
            return 2;
        }
        else if (a == "--signals") { while (i + 1 < argc && !is_flag(argv[i + 1])) signals.push_back(argv[++i]); }
        else return usage();
    }
    if (signals.empty()) {
        fprintf(stderr, "--signals <files|dirs|tt.csv>... is required\n");
        return usage();
    }
    if (P < 1 || P > 80) { fprintf(stderr, "-P %d: prediction order out of range [1, 80]\n", P); return 2; }
    if (O < 1 || W < 1) { fprintf(stderr, "-W and -O must be positive\n"); return 2; }
    // utl::resolve_files3(&signals, tt, &class, "", signals_dir_template, ".wav") (src/lpc/mod.rs:103-110)
    std::vector<std::string> files;
    const bool tt_list = signals.size() == 1 && signals[0].size() > 4 &&
                         signals[0].compare(signals[0].size() - 4, 4, ".csv") == 0;
    int rc = tt_list ? e2vq_io::files_from_csv(signals[0], tt, cls, "", ".wav", &tmpl, files)
                     : e2vq_io::resolve_filenames(signals, ".wav", files);
    if (rc) { printf("%s\n", e2vq_last_error()); return 0; }
    auto ptrs = cptrs(files);
    return ecoz2_lpc_signals(P, W, O, minpc, split, ptrs.data(), (int)ptrs.size(), mintrpt, verbose ? 1 : 0) ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "cversion")) {
        printf("%s\n", ecoz2_version());
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "seq") && !strcmp(argv[2], "show")) return seq_show(argc - 3, argv + 3);
    if (argc >= 3 && !strcmp(argv[1], "prd") && !strcmp(argv[2], "show")) return prd_show(argc - 3, argv + 3);
    if (argc >= 2 && !strcmp(argv[1], "lpc")) return lpc_cmd(argc - 2, argv + 2);
    if (argc >= 3 && !strcmp(argv[1], "hmm")) return hmm_cmd(argc - 2, argv + 2);
    if (argc >= 3 && !strcmp(argv[1], "nb")) return seq_model_cmd(true, argc - 2, argv + 2);
    if (argc >= 3 && !strcmp(argv[1], "mm")) return seq_model_cmd(false, argc - 2, argv + 2);
    if (argc < 3 || strcmp(argv[1], "vq") != 0) return usage();
    const std::string cmd = argv[2];
    if (cmd == "learn") return vq_learn(argc - 3, argv + 3);
    if (cmd == "quantize") return vq_quantize(argc - 3, argv + 3);
    if (cmd == "classify") return vq_classify(argc - 3, argv + 3);
    if (cmd == "show") return vq_show(argc - 3, argv + 3);
    return usage();
}
