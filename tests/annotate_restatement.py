"""Test infrastructure: phaser_annotate's four steps restated over plain dicts and lists (the checker of phaser_amd/annotate.py and K_annot, never
part of the product).  It is fed with CADD and allele-frequency rows that somebody else has already looked up, so it needs no index reader.

Tables (what the reference keeps in its module globals):
  gw_info / pg_info   {variant id: [two allele indices, annotations, gene list, block]}; annotations = {"gene:alt_index": [phred, effect, gene id,
                      gene name, contig, position, allele frequency or None, alt base]}
  gw_genes / pg_genes {gene: [variant id, ...]} -- a variant once per matching CADD row
  gene_order          genes by first appearance (the project's stated order; the reference iterates a set)
  rsid                {variant id: ID column}
  af                  {"contig_pos_alt": value} with an allele-frequency VCF, else None
"""


def _info_fields(text):
    out = {}
    for item in text.split(";"):
        if "=" in item:
            out[item.split("=")[0]] = item.split("=")[1]
    return out


def _alleles_of(field, slash_allowed):
    """-> None when the variant is not taken, "skip" when it would be taken but is not two one-digit alleles, else [a0, a1]"""
    chars = list(field)
    if "." in chars or chars.count("0") == 2:
        return None
    if "/" in chars and not slash_allowed:
        return None
    left = list(chars)
    for sep in ("/", "|"):
        if sep in left:
            left.remove(sep)
    if "|" not in chars and len(set(left)) != 1:
        return None
    if len(left) != 2 or not all(x.isdigit() and len(x) == 1 for x in left):
        return "skip"
    return [int(left[0]), int(left[1])]


def annotations_of(uid, info, cadd_rows, af_field):
    """one variant's CADD rows -> (annotations, gene list); cadd_rows = {(contig, pos): [all fields of a row, ...]}"""
    contig, pos, _, alt_text = uid.split("_")
    alts = alt_text.split(",")
    notes, genes = {}, []
    for row in cadd_rows.get((contig, int(pos)), []):
        if int(row[1]) != int(pos) or row[4] not in alts:
            continue
        index = alts.index(row[4]) + 1
        genes.append(row[92])
        freq = None
        if af_field is not None and af_field in info:
            parts = info[af_field].split(",")
            if index - 1 < len(parts):
                try:
                    freq = float(parts[index - 1])
                except ValueError:
                    freq = None
        notes["%s:%d" % (row[92], index)] = [row[-1], row[10], row[92], row[95], contig, int(pos), freq, row[4]]
    return notes, genes


def build_tables(vcf_text, sample, cadd_rows, af_rows=None, af_field="AF"):
    """Steps 1-3.  af_rows = None: frequencies come from the genotype VCF's INFO; else {(contig, pos): [(ALT text, INFO text), ...]} of the
    allele-frequency VCF in file order.  Raises ValueError("sample") when the sample is not in the header."""
    gw_wanted, pg_wanted, rsid = [], [], {}
    skipped = 0
    column = 0
    for line in vcf_text.split("\n"):
        if line.startswith("#CHR"):
            names = line.split("\t")
            if sample not in names:
                raise ValueError("sample")
            column = names.index(sample)
            continue
        if not line or line.startswith("#"):
            continue
        c = line.split("\t")
        uid = "_".join([c[0], c[1], c[3], c[4]])
        rsid[uid] = c[2]
        keys, values = c[8].split(":"), c[column].split(":")
        if len(keys) != len(values):
            continue
        info = _info_fields(c[7])
        if "GT" in keys:
            al = _alleles_of(values[keys.index("GT")], True)
            if al == "skip":
                skipped += 1
            elif al is not None:
                gw_wanted.append((uid, info, al, 0.0))
        if "PG" in keys and "PI" in keys:
            al = _alleles_of(values[keys.index("PG")], False)
            if al == "skip":
                skipped += 1
            elif al is not None:
                pg_wanted.append((uid, info, al, float(values[keys.index("PI")])))
    field = af_field if af_rows is None else None
    T = {"gw_info": {}, "pg_info": {}, "gw_genes": {}, "pg_genes": {}, "gene_order": [], "rsid": rsid, "af": None, "skipped": skipped}

    seen = set()

    def enlist(which, gene, uid):
        if gene not in seen:
            seen.add(gene)
            T["gene_order"].append(gene)
        T[which].setdefault(gene, []).append(uid)

    for uid, info, al, block in gw_wanted:
        notes, genes = annotations_of(uid, info, cadd_rows, field)
        T["gw_info"][uid] = [al, notes, genes, 0.0]
        for gene in genes:
            enlist("gw_genes", gene, uid)
    known = set(T["gw_info"])
    rest = []
    for item in pg_wanted:
        uid = item[0]
        if uid in known:
            T["pg_info"][uid] = T["gw_info"][uid]
            for gene in T["gw_info"][uid][2]:
                enlist("pg_genes", gene, uid)
        else:
            rest.append(item)
    for uid, info, al, block in rest:
        notes, genes = annotations_of(uid, info, cadd_rows, field)
        T["pg_info"][uid] = [al, notes, genes, block]
        for gene in genes:
            enlist("pg_genes", gene, uid)
    if af_rows is not None:
        T["af"] = {}
        for table in (T["gw_info"], T["pg_info"]):
            for uid, rec in table.items():
                for note in rec[1].values():
                    contig, pos, base = note[4], note[5], note[7]
                    value = 0
                    found = af_rows.get((contig, pos), [])
                    if found:
                        alts = found[0][0].split(",")
                        text = _info_fields(found[0][1]).get(af_field, "")
                        freqs = text.split(",") if text else []
                        if base in alts and alts.index(base) < len(freqs):
                            value = float(freqs[alts.index(base)])
                    T["af"]["%s_%d_%s" % (contig, pos, base)] = value
    return T


def combinations(one, other):
    """[allele of one, allele of other, "cis" / "trans"] for the two info records of one phase block, reference alleles left out"""
    found = []
    if one[3] == other[3]:
        for i in range(len(one[0])):
            for j in range(len(one[0])):
                found.append([int(one[0][i]), int(other[0][j]), "cis" if i == j else "trans"])
    return [f for f in found if f[0] != 0 and f[1] != 0]


def rows_of(T, gene, uid_a, rec_a, uid_b, rec_b, combos, read_backed):
    out = []
    for allele_a, allele_b, config in combos:
        key_a, key_b = "%s:%d" % (gene, allele_a), "%s:%d" % (gene, allele_b)
        if key_a not in rec_a[1] or key_b not in rec_b[1]:
            continue
        na, nb = rec_a[1][key_a], rec_b[1][key_b]
        shown_a, shown_b, af_a, af_b = allele_a, allele_b, ".", "."
        if T["af"] is not None:
            shown_a, shown_b = na[7], nb[7]
            af_a = T["af"]["%s_%d_%s" % (na[4], na[5], na[7])]
            af_b = T["af"]["%s_%d_%s" % (nb[4], nb[5], nb[7])]
        else:
            if na[6] is not None:
                af_a = na[6]
            if nb[6] is not None:
                af_b = nb[6]
        out.append([gene, na[3], uid_a, T["rsid"].get(uid_a, "."), shown_a, af_a, na[0], na[1], uid_b, T["rsid"].get(uid_b, "."), shown_b, af_b, nb[0], nb[1],
                    config, read_backed])
    return out


def gene_rows(T, gene):
    """Step 4 for one gene: the genome-wide pass, then the read-backed pass over what the first did not put out"""
    out = []
    done = set()
    gw_list, pg_list = T["gw_genes"].get(gene, []), T["pg_genes"].get(gene)
    for a in gw_list:
        for b in gw_list:
            if a == b:
                continue
            gw = combinations(T["gw_info"][a], T["gw_info"][b])
            rb = []
            if pg_list is not None and a in pg_list and b in pg_list:
                rb = combinations(T["pg_info"][a], T["pg_info"][b])
            verdict = "0"
            if len(gw) == len(rb) and gw == rb:
                verdict = "1"
            if len(gw) == len(rb) and gw != rb:
                verdict = "-1"
            elif len(rb) == 0:
                verdict = "0"
            out += rows_of(T, gene, a, T["gw_info"][a], b, T["gw_info"][b], gw, verdict)
            if verdict == "-1":
                out += rows_of(T, gene, a, T["gw_info"][a], b, T["gw_info"][b], rb, "1")
            done.add((a, b))
    for a in pg_list or []:
        for b in pg_list:
            if a != b and (a, b) not in done:
                out += rows_of(T, gene, a, T["pg_info"][a], b, T["pg_info"][b], combinations(T["pg_info"][a], T["pg_info"][b]), "1")
                done.add((a, b))
    return out


def all_rows(T):
    out = []
    for gene in T["gene_order"]:
        if gene != "NA":
            out += gene_rows(T, gene)
    return out


HEADER = ["ensg", "name", "variant_a", "rsid_a", "allele_a", "af_a", "cadd_phred_a", "cadd_effect_a", "variant_b", "rsid_b", "allele_b", "af_b",
          "cadd_phred_b", "cadd_effect_b", "configuration", "read_backed"]


def text_of(rows):
    return "".join("\t".join(map(str, r)) + "\n" for r in [HEADER] + rows)


def record_tuples(rows):
    """(gene, variant a, variant b, allele a, allele b, configuration, read_backed) of rows made WITHOUT an allele-frequency VCF"""
    return [(r[0], r[2], r[8], int(r[4]), int(r[10]), r[14], int(r[15])) for r in rows]


def pair_count(T):
    return sum(len(T["gw_genes"].get(g, [])) ** 2 + len(T["pg_genes"].get(g, [])) ** 2 for g in T["gene_order"] if g != "NA")
