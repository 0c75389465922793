// TopologySearch.h: the events a topology search sends and the interface of a search.
#ifndef BPP_AMD_TOPOLOGYSEARCH_H
#define BPP_AMD_TOPOLOGYSEARCH_H

namespace bpp {

class TopologySearch;

// What a listener is told about a change (the search that made it; may be null)
class TopologyChangeEvent {
  const TopologySearch* source_ = nullptr;

 public:
  TopologyChangeEvent() {}
  explicit TopologyChangeEvent(const TopologySearch& source) : source_(&source) {}
  const TopologySearch* getTopologySearch() const { return source_; }
};

// Told when a change was tried (Tested), was kept (Successful), or was applied to the tree
// (Performed).  The defaults do nothing.
class TopologyListener {
 public:
  virtual ~TopologyListener() {}
  virtual void topologyChangeTested(const TopologyChangeEvent&) {}
  virtual void topologyChangeSuccessful(const TopologyChangeEvent&) {}
  virtual void topologyChangePerformed(const TopologyChangeEvent&) {}
};

class TopologySearch {
 public:
  virtual ~TopologySearch() {}
  virtual void search() = 0;
  // not owned
  virtual void addTopologyListener(TopologyListener* listener) = 0;
};

}  // namespace bpp

#endif
